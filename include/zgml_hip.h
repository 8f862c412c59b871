/*
 * zgml_hip.h — C ABI of the MI355X (gfx950) backend for zgml's forward-inference path.
 *
 * This header is the drop-in boundary. Every entry point replaces one slot of the
 * reference's backend plugin surface (all citations relative to the zgml tree):
 *
 *   zgml_hip_create / zgml_hip_destroy   <-> Backend.ctx lifetime           src/backend.zig:330-336
 *   zgml_hip_dense_matmul_f32            <-> VTable.dense_matmul_f32        src/backend.zig:341
 *   zgml_hip_compile_program             <-> VTable.compile_program         src/backend.zig:343
 *   zgml_hip_refresh_program             <-> VTable.refresh_program         src/backend.zig:345
 *   zgml_hip_execute_program             <-> VTable.execute_program         src/backend.zig:347
 *   zgml_hip_free_program                <-> VTable.free_program            src/backend.zig:349
 *   zgml_hip_get_runtime_profile         <-> VTable.get_runtime_profile     src/backend.zig:351
 *   zgml_hip_capabilities                <-> Backend.capabilities           src/backend.zig:14-141
 *   zgml_hip_program_supported           <-> DeviceProgram.isSupportedBy    src/backend.zig:277-325
 *
 * The structs below mirror the Zig types field for field (zgml_device_op <-> DeviceOp
 * src/backend.zig:179-249, zgml_program_io <-> ProgramIO :252-257, zgml_qweight_upload <->
 * QuantizedWeightUpload :260-266, zgml_device_program <-> DeviceProgram :270-275). Zig slices
 * become (pointer, length) pairs and the tagged union becomes `kind` + a C union, so a Zig
 * adapter can fill them with `extern struct`s (INTEGRATION.md shows it).
 *
 * Plain C: no C++ types, no torch types, no HIP types in any signature. Offsets and strides of
 * device ops are in f32 ELEMENTS; zgml_program_io offsets/sizes are in BYTES; buffer_sizes are
 * f32 element counts (same units as the reference).
 *
 * Extension entry points (zgml_hip_*_ext, zgml_hip_qmatvec_bench_*) have no reference
 * counterpart; they exist for measurement and for the row-sharded multi-GPU path and are marked
 * as such below.
 */
#ifndef ZGML_HIP_H
#define ZGML_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZGML_HIP_ABI_VERSION 1

/* ── Op enum ordinals: src/op.zig:11-62 (graph IR `Op`) ─────────────────────────────────── */
enum {
    ZGML_OP_NONE = 0,
    ZGML_OP_VIEW = 1,
    ZGML_OP_RESHAPE = 2,
    ZGML_OP_TRANSPOSE = 3,
    ZGML_OP_PERMUTE = 4,
    ZGML_OP_AS_STRIDED = 5,
    ZGML_OP_BROADCAST_TO = 6,
    ZGML_OP_ADD = 7,
    ZGML_OP_MUL = 8,
    ZGML_OP_NEG = 9,
    ZGML_OP_ABS = 10,
    ZGML_OP_SGN = 11,
    ZGML_OP_STEP = 12,
    ZGML_OP_RELU = 13,
    ZGML_OP_SQRT = 14,
    ZGML_OP_RECIP = 15,
    ZGML_OP_EXP = 16,
    ZGML_OP_LOG = 17,
    ZGML_OP_GELU = 18,
    ZGML_OP_SUM = 19,
    ZGML_OP_MAX = 20,
    ZGML_OP_REPEAT = 21
};

/* ── DeviceOp tags, in the declaration order of the Zig union (src/backend.zig:179-249) ──── */
enum {
    ZGML_DOP_ELEMENTWISE = 0,
    ZGML_DOP_MATMUL = 1,
    ZGML_DOP_QMATMUL = 2,
    ZGML_DOP_SOFTMAX = 3,
    ZGML_DOP_LAYERNORM = 4,
    ZGML_DOP_RMSNORM = 5,
    ZGML_DOP_REDUCE = 6,
    ZGML_DOP_REPEAT = 7,
    ZGML_DOP_SLICE_ASSIGN = 8,
    ZGML_DOP_ROPE = 9,
    ZGML_DOP_ATTENTION = 10,
    ZGML_DOP_FUSED_ELEMENTWISE = 11,
    ZGML_DOP_COUNT = 12,
    /* Extension kinds (no reference DeviceOp): the quantised KV cache of
     * src/quant.zig:645-1091 as device ops. Never counted in the reference-shaped profile arrays. */
    ZGML_DOP_KVQ_STORE = 13,     /* QuantizedKVCache.storeColumn */
    ZGML_DOP_ATTENTION_KVQ = 14  /* attentionQuantized */
};

/* MatMulGeometry, src/backend.zig:146-158 (usize -> uint64_t). */
typedef struct zgml_matmul_geom {
    uint64_t M, N, K;
    uint64_t a_row_stride, a_col_stride;
    uint64_t b_row_stride, b_col_stride;
    uint64_t a_offset, b_offset;
    uint64_t dst_offset, dst_row_stride;
} zgml_matmul_geom;

/* FusedEwStep, src/backend.zig:170-175. */
typedef struct zgml_fused_step {
    uint32_t op;               /* ZGML_OP_* */
    uint8_t is_swapped;        /* chain value sits in the src1 position */
    uint8_t _pad;
    uint16_t secondary_buf;    /* external operand of a binary step */
    uint32_t secondary_offset; /* elements */
} zgml_fused_step;

typedef struct zgml_op_elementwise {
    uint32_t op;
    uint16_t dst, src0, src1, _pad;
    uint32_t n, dst_offset, src0_offset, src1_offset;
} zgml_op_elementwise;

typedef struct zgml_op_matmul {
    uint16_t dst, a, b, _pad;
    zgml_matmul_geom geom;
} zgml_op_matmul;

typedef struct zgml_op_qmatmul {
    uint16_t dst, input, weight_idx, _pad;
    uint32_t M, N, K;
    uint32_t input_offset, input_row_stride; /* stride 0 => K */
    uint32_t dst_offset, dst_row_stride;     /* stride 0 => N */
} zgml_op_qmatmul;

typedef struct zgml_op_rowwise { /* softmax / layernorm / rmsnorm */
    uint16_t dst, src;
    uint32_t rows, cols;
    float eps; /* ignored by softmax */
    uint32_t src_offset, dst_offset;
} zgml_op_rowwise;

typedef struct zgml_op_reduce {
    uint32_t op; /* ZGML_OP_SUM or ZGML_OP_MAX */
    uint16_t dst, src;
    uint32_t n_out, reduce_size;
    uint32_t src_offset, dst_offset;
} zgml_op_reduce;

typedef struct zgml_op_repeat {
    uint16_t dst, src;
    uint32_t n;
    uint32_t src_ne[4], dst_ne[4], src_strides[4], dst_strides[4];
    uint32_t src_offset, dst_offset;
} zgml_op_repeat;

typedef struct zgml_op_slice_assign {
    uint16_t dst, src;
    uint32_t rows, cols;
    uint32_t dst_base_offset;
    uint32_t dst_offset; /* dynamic: dst_base_offset + pos * patch_stride */
    uint32_t dst_row_stride, dst_col_stride;
    uint32_t src_offset, src_row_stride, src_col_stride;
    uint32_t patch_stride; /* 0 => static */
} zgml_op_slice_assign;

typedef struct zgml_op_rope {
    uint16_t dst, src, cos_sin, _pad;
    uint32_t half_d, seq_len;
    uint32_t src_off, cs_off, dst_off;
    uint32_t src_rs, src_cs, cs_cs;
} zgml_op_rope;

typedef struct zgml_op_attention {
    uint16_t dst, q, k, v, mask;
    uint8_t has_mask, _pad;
    uint32_t d_head, seq_q;
    uint32_t seq_kv; /* dynamic */
    float scale;
    uint32_t q_off, k_off, v_off, mask_off, dst_off;
    uint32_t q_rs, q_cs, k_rs, k_cs, v_rs, v_cs, mask_rs, mask_cs, dst_rs, dst_cs;
} zgml_op_attention;

/* A quantised KV cache lives in ONE program buffer (f32-element sized like every buffer):
 *   int8 q_data[n_cols * d_head]            column c at byte offset c * d_head
 *   f32  scales[n_cols * d_head/block_size] at element offset n_cols * d_head / 4, column-major
 * so buffer_sizes[cache] >= n_cols*d_head/4 + n_cols*d_head/block_size (n_cols*d_head % 4 == 0). */

/* QuantizedKVCache.storeColumn (src/quant.zig:687-699 -> quantizeInput :320-341): quantise the d_head
 * f32 values at src[src_offset ..] (unit stride) into column `col`. `col` is the dynamic field
 * (refresh: col_base + pos * patch_stride, like slice_assign.dst_offset). */
typedef struct zgml_op_kvq_store {
    uint16_t cache, src;
    uint32_t d_head, block_size, n_cols;
    uint32_t src_offset;
    uint32_t col_base;
    uint32_t col; /* dynamic */
    uint32_t patch_stride;
} zgml_op_kvq_store;

/* attentionQuantized (src/quant.zig:925-1091): q / dst dense f32 columns (unit row stride), K and V
 * columns [k_col_start, k_col_start + seq_kv) / [v_col_start, ...) of two quantised caches, optional
 * additive mask, streaming softmax; a query with no valid key yields zeros. */
typedef struct zgml_op_attention_kvq {
    uint16_t dst, q, k, v, mask;
    uint8_t has_mask, _pad;
    uint32_t d_head, seq_q;
    uint32_t seq_kv; /* dynamic */
    float scale;
    uint32_t block_size, n_cols;
    uint32_t k_col_start, v_col_start;
    uint32_t q_off, q_cs, dst_off, dst_cs;
    uint32_t mask_off, mask_rs, mask_cs;
} zgml_op_attention_kvq;

typedef struct zgml_op_fused_elementwise {
    const zgml_fused_step* steps; /* borrowed: must outlive the compiled program's use of `ops` */
    uint32_t n_steps;
    uint32_t n;
    uint16_t dst, src;
    uint32_t dst_offset, src_offset;
} zgml_op_fused_elementwise;

/* DeviceOp, src/backend.zig:179-249. */
typedef struct zgml_device_op {
    uint32_t kind; /* ZGML_DOP_* */
    uint32_t _pad;
    union {
        zgml_op_elementwise elementwise;
        zgml_op_matmul matmul;
        zgml_op_qmatmul qmatmul;
        zgml_op_rowwise softmax;
        zgml_op_rowwise layernorm;
        zgml_op_rowwise rmsnorm;
        zgml_op_reduce reduce;
        zgml_op_repeat repeat;
        zgml_op_slice_assign slice_assign;
        zgml_op_rope rope;
        zgml_op_attention attention;
        zgml_op_fused_elementwise fused_elementwise;
        zgml_op_kvq_store kvq_store;         /* extension */
        zgml_op_attention_kvq attention_kvq; /* extension */
    } u;
} zgml_device_op;

/* ProgramIO, src/backend.zig:252-257. offset/size in bytes. */
typedef struct zgml_program_io {
    uint16_t buf_idx;
    uint16_t _pad;
    uint32_t offset;
    void* host_ptr;
    uint32_t size;
    uint32_t _pad2;
} zgml_program_io;

/* QuantizedWeightUpload, src/backend.zig:260-266: int8 data in flat [K,N] row-major order
 * (index k*N+n), one f32 scale per `block_size` consecutive FLAT elements.
 *
 * Extension (no reference counterpart yet): the packed-GGUF pass-through form. With
 * `scales == NULL && scales_len == 0 && block_size == 32`, `data` holds the tensor's GGUF blocks exactly
 * as they sit in the file — block b covers flat elements [32b, 32b+32) —
 *     data_len == rows*cols/32 * 18  ->  Q4_0 blocks {f16 scale, 16 bytes}; element j of the block is the
 *                                        low (j even) / high (j odd) nibble of byte j/2, value = nibble - 8
 *                                        — the reference loader's interleaved order (gguf_loader.zig:137-141)
 *     data_len == rows*cols/32 * 34  ->  Q8_0 blocks {f16 scale, 32 int8}
 * i.e. what quantizedWeightFromInfo (src/models/gguf_loader.zig:99-154) expands on the host; here the
 * expansion and the re-pack happen on the device and half (Q4_0) of the bytes cross PCIe.
 * Requires rows*cols % 32 == 0 and cols % 32 == 0. */
#define ZGML_QW_GGUF_Q4_0_BLOCK_BYTES 18
#define ZGML_QW_GGUF_Q8_0_BLOCK_BYTES 34
typedef struct zgml_qweight_upload {
    const int8_t* data;
    uint64_t data_len;
    const float* scales;
    uint64_t scales_len;
    uint64_t rows; /* K */
    uint64_t cols; /* N */
    uint64_t block_size;
} zgml_qweight_upload;

/* DeviceProgram, src/backend.zig:270-275. */
typedef struct zgml_device_program {
    const zgml_device_op* ops;
    uint64_t n_ops;
    uint16_t n_buffers;
    const uint64_t* buffer_sizes; /* f32 elements, n_buffers entries */
    uint64_t n_buffer_sizes;
    const zgml_program_io* initial_uploads;
    uint64_t n_initial_uploads;
    const zgml_qweight_upload* qweights;
    uint64_t n_qweights;
} zgml_device_program;

/* Capabilities, src/backend.zig:14-58. Optionals: *_has = 0 means "null" (no limit). */
typedef struct zgml_capabilities {
    uint8_t compiled_programs;
    uint8_t host_visible_program_memory;
    uint8_t dense_matmul_f32;
    uint8_t dense_matmul_f16;
    uint8_t qmatmul;
    uint8_t fused_elementwise;
    uint8_t f16_weight_promotion;
    uint8_t dynamic_program_refresh;
    uint8_t prefill_attention;
    uint8_t decode_attention;
    uint8_t quantized_kv;
    uint8_t command_buffer_execution;
    uint8_t max_fused_elementwise_steps_has;
    uint8_t attention_supported;
    uint8_t attention_max_seq_kv_has;
    uint8_t attention_max_d_head_has;
    uint32_t max_fused_elementwise_steps;
    uint32_t attention_max_seq_kv;
    uint32_t attention_max_d_head;
} zgml_capabilities;

/* Subset of profile.RuntimeProfile (src/profile.zig:820-843) a device backend can fill. */
typedef struct zgml_runtime_profile {
    uint64_t time_ns[ZGML_DOP_COUNT]; /* per DeviceOp tag; filled only in profiling mode */
    uint64_t backend_op_count;
    uint64_t fallback_op_count; /* always 0: there is no CPU fallback */
    uint64_t backend_dispatch_count;
    uint64_t sync_time_ns;
    uint64_t sync_count;
    uint32_t call_count;
    uint32_t _pad;
} zgml_runtime_profile;

typedef struct zgml_hip_ctx zgml_hip_ctx;         /* Backend.ctx */
typedef struct zgml_hip_program zgml_hip_program; /* Backend.CompiledHandle */

/* Create a backend context on HIP device `device_ordinal`. NULL on failure (no device, not
 * gfx950, allocation failure); zgml_hip_last_error(NULL) then describes why. */
zgml_hip_ctx* zgml_hip_create(int device_ordinal);
void zgml_hip_destroy(zgml_hip_ctx* ctx);

/* Sticky, human-readable description of the first error recorded on the context (or of the
 * last failed zgml_hip_create when ctx == NULL). Empty string when there is none. The vtable has
 * no error channel on execute (src/backend.zig:347 returns void), hence the side channel. */
const char* zgml_hip_last_error(const zgml_hip_ctx* ctx);
void zgml_hip_clear_error(zgml_hip_ctx* ctx);

/* Capabilities.hip — what DeviceInference consults when lowering (src/device_inference.zig:108). */
void zgml_hip_capabilities(zgml_capabilities* out);

/* DeviceProgram.isSupportedBy(Capabilities.hip): 1 if supported, else 0. Pure host logic. */
int zgml_hip_program_supported(const zgml_device_program* program);

/* VTable.dense_matmul_f32: host slices in, result in dst on return. Returns 1 if handled,
 * 0 to make the caller fall back (src/tensor/forward.zig:2022-2031). dst_len/a_len/b_len are
 * element counts of the host slices. */
int zgml_hip_dense_matmul_f32(zgml_hip_ctx* ctx, float* dst, uint64_t dst_len, const float* a,
                              uint64_t a_len, const float* b, uint64_t b_len,
                              const zgml_matmul_geom* geom);

/* VTable.compile_program. Every array is borrowed for the duration of the call only: the backend
 * copies the op list (including fused steps), so the caller may free everything afterwards (the
 * reference's cpu/metal backends keep `ops` borrowed, src/backend/cpu.zig:115; copying is a
 * superset of that contract). Returns NULL on failure or when the program is unsupported. */
zgml_hip_program* zgml_hip_compile_program(zgml_hip_ctx* ctx, const zgml_device_program* program);

/* VTable.refresh_program: same-length op list whose dynamic fields changed
 * (slice_assign.dst_offset, attention.seq_kv). Other fields must be unchanged. */
void zgml_hip_refresh_program(zgml_hip_ctx* ctx, zgml_hip_program* handle,
                              const zgml_device_op* ops, uint64_t n_ops);
/* (extension, round 5) Outputs written straight into the caller's buffer. By default execute_program lands outputs in the
 * library's pinned staging buffer and copies them to `host_ptr` (197 KB of logits per SmolLM-135M token). With on = 1 a program
 * whose execute_program calls name ONE output at the SAME host address three times in a row registers that buffer with the
 * driver (hipHostRegister) and the step's last kernel writes into it. THE CALLER PROMISES that such a buffer stays allocated
 * and mapped until it passes a different address, switches this off, or frees the program: pages are pinned at registration,
 * so a buffer that is freed and re-allocated at the same address would silently stop receiving data. DeviceInference's
 * session-owned logits slice (src/device_inference.zig:262) qualifies. Returns 0. */
int zgml_hip_program_pin_outputs(zgml_hip_ctx* ctx, zgml_hip_program* program, int on);

/* The per-token refresh reduced to its two numbers (src/backend/program.zig:7452-7490 StepDynamicParams, what the reference's wgpu
 * backend uploads per step, src/backend/wgpu.zig:1162-1169): every dynamic KV store goes to column `slice_pos` (dst_offset =
 * dst_base_offset + slice_pos * patch_stride), every attention reads `seq_kv` keys. O(#dynamic ops) instead of a compare of the
 * whole op list; static fields are not examined — an adapter derives (slice_pos, seq_kv) with stepDynamicStateFromOps and calls
 * this when `needsUpload()`, and calls zgml_hip_refresh_program (which detects static changes and rebuilds) otherwise.
 * Returns 0, -1 on a null argument. */
int zgml_hip_refresh_dynamic(zgml_hip_ctx* ctx, zgml_hip_program* handle, uint32_t slice_pos, uint32_t seq_kv);

/* VTable.execute_program: upload inputs, run all ops in order, download outputs; blocking. */
void zgml_hip_execute_program(zgml_hip_ctx* ctx, zgml_hip_program* handle,
                              const zgml_program_io* inputs, uint64_t n_inputs,
                              const zgml_program_io* outputs, uint64_t n_outputs);

void zgml_hip_free_program(zgml_hip_ctx* ctx, zgml_hip_program* handle);

/* VTable.get_runtime_profile: pointer stays valid until free_program. */
zgml_runtime_profile* zgml_hip_get_runtime_profile(zgml_hip_ctx* ctx, zgml_hip_program* handle);

/* ── Extensions (no reference counterpart) ──────────────────────────────────────────────── */

/* The launch plan of a program as text, one line per launch, for diagnostics and tests (which ops a launch covers, and for
 * a quantized mat-vec launch its parts, K, prologue form — none | mul | rmsnorm | prenorm —, whether it prepares the NEXT
 * launch's norm, carries the gate / up pair product or the decode attention of its heads). Builds the plan if it is not
 * built yet. Writes at most cap - 1 bytes + NUL; returns the bytes the whole text needs (without the NUL). */
uint64_t zgml_hip_program_plan_text(zgml_hip_ctx* ctx, zgml_hip_program* handle, char* out, uint64_t cap);

/* Program options, set before compile on the context. */
enum {
    ZGML_HIP_OPT_FUSION = 1,         /* 0/1: pattern-fuse the op stream (default 1) */
    ZGML_HIP_OPT_GRAPH = 2,          /* 0/1: replay a captured hipGraph per execute (default 1) */
    ZGML_HIP_OPT_PROFILE = 3,        /* 0/1: per-op hipEvent timing into time_ns (default 0) */
    ZGML_HIP_OPT_SKIP_DEAD_UPLOADS = 4, /* 0/1: do not allocate/upload buffers no op touches (default 1) */
    ZGML_HIP_OPT_F16_DENSE_WEIGHTS = 5, /* 0/1: f16 weight promotion for dense matmul B (default 0) */
    /* bytes (0 = off, default): zgml_hip_dense_matmul_f32 keeps device copies of its B operands, keyed by
     * host pointer, up to this many bytes (plain ComputeGraph.compute() users whose
     * weights never move). The caller promises B is not mutated between calls, or invalidates. */
    ZGML_HIP_OPT_DENSE_WEIGHT_CACHE = 6,
    /* keys per workgroup at which a fused decode attention starts to split one head's context over
     * several workgroups (flash-decoding split; default 128, minimum 32, 0 = never split). A head splits
     * once seq_kv >= 2 * value; below that the launch behaves exactly as without the option. */
    ZGML_HIP_OPT_ATTN_SPLIT_MIN_KEYS = 7,
    /* workgroups (1024 threads) the device is assumed to keep resident at once, for the launch that carries the q/k/v
     * projection AND the decode attention that waits for it in one grid (the waiting workgroups spin on workgroups of the
     * same grid, so the whole grid must be resident): the fusion is only built when projection + attention workgroups fit,
     * the attention's split count shrinks to fit, otherwise the two launches stay apart. -1 (default): one 1024-thread workgroup
     * per compute unit for the short-K form; the 256-thread K-on-lanes form (K > 2048: Llama-2-7B) takes what the occupancy
     * query admits (four per compute unit, no margin) and is only built with ALL the splits the stand-alone attention would
     * use. 0: never fuse. Takes effect for programs compiled afterwards and at the next plan rebuild of existing ones.
     * A hand-off wait that gives up is bounded and reported at the next host synchronisation (sticky error on the context): the
     * results of THAT execution are wrong, including the KV-cache column it wrote — re-run the step at the same position (the
     * context has switched the fusion off and rebuilt the plan, the re-run rewrites the column); nothing older is affected. */
    ZGML_HIP_OPT_FUSE_RESIDENT_WGS = 8,
    /* 0/1 (default 0; the environment variable ZGML_HIP_KSPLIT=1 turns it on for every context): the decoder layer of a short-K
     * model (K <= 2048, Q4_0 weights with f16 scales, d_head 64 / 128) as launches that end at a K-split instead of an all-to-all
     * seam — each head's attention workgroup adds its partial of the O projection, each 32-column gate / up workgroup its partial
     * of the down projection, the next launch sums the partials in its prologue (zgml_amd/csrc/ksplit.hip). Same results within the
     * mat-vec tolerance, two launches per layer instead of four — and MEASURED SLOWER on MI355X (DESIGN.md section 4, round 5:
     * reading 48 partial vectors costs a consumer workgroup more than the launch boundary it replaces), hence off by default.
     * Latched per program at compile_program. */
    ZGML_HIP_OPT_KSPLIT = 9,
    /* 0/1 (default 0; ZGML_HIP_W8A8 in the environment): M = 1 qmatmuls take the reference's W8A8 arm — what its CPU executor does
     * when a weight carries a transposed image (src/backend/reference.zig:512-528): quantizeInput on the input row (int8 + one f32
     * scale per 32 values, src/quant.zig:604-640), the weight re-quantised per (column, 32 k) as prepareTransposed does
     * (src/quant.zig:560-603; done on the device at compile_program from the int8 + f32-scale upload) and gemvRange's block-ordered
     * f32 combine of int32 dots (src/quant.zig:320-440). BIT-IDENTICAL to that arm (zgml_amd/csrc/w8a8.hip); it is NOT the exact
     * dequantise-then-dot arithmetic the default path (and the reference's x86 / GPU backends) computes: results differ by the
     * activations' int8 rounding. Applies to weights of block size 32 with K % 64 == 0, K <= 16384, N % 16 == 0 every use of which
     * is a dense M = 1 row; such ops run unfused. Read at compile_program. */
    ZGML_HIP_OPT_W8A8 = 10,
    /* 0 (default) / 1 / 2..8: quantized matmuls of 2 <= M <= bound rows (batched decode: one row per sequence) over Q4_0 weights
     * with f16 scales and K >= the K-on-lanes threshold take the multi-row K-on-lanes mat-vec (zgml_amd/csrc/qmatvec_rows.hip)
     * instead of the MFMA tile kernels. 1: bound = 6, the largest M at which that kernel measured faster than the tile kernels at
     * Llama-2-7B size; 2..8: that bound (the kernel exists up to 8 rows). Such a weight is packed K-on-lanes
     * when EVERY qmatmul over it has M <= bound (without the option: M = 1), and a later refresh that raises M above the bound over
     * it is refused. Same results within the mat-vec tolerance. Short-K weights keep the n-on-lanes layout and the tile kernels.
     * Read at compile_program. */
    ZGML_HIP_OPT_SMALL_M_MATVEC = 11,
    /* 0 (default) / 1: zgml_hip_kv_move's 16-byte loads (and, in the copying forms, its 16-byte stores) are non-temporal; the
     * dword path of unaligned lanes and the few dwords behind a chunk's last 16 bytes stay plain. Measured at Llama-2-7B lanes
     * (DESIGN.md section 4.9): no difference. Read at every call. */
    ZGML_HIP_OPT_KV_MOVE_NT = 12
};
int zgml_hip_set_option(zgml_hip_ctx* ctx, int option, int64_t value);
/* Drop the cached device copy of host operand `b` (NULL: all of them). */
void zgml_hip_dense_cache_invalidate(zgml_hip_ctx* ctx, const float* b);
void zgml_hip_dense_cache_stats(zgml_hip_ctx* ctx, uint64_t* hits, uint64_t* misses, uint64_t* bytes);

/* Raw device access for harnesses that keep data resident (bench, multi-GPU all-gather glue):
 * device pointer of program buffer `buf_idx` (NULL if elided). */
void* zgml_hip_program_buffer_ptr(zgml_hip_program* handle, uint16_t buf_idx);
/* Device-to-device copy of n_elems f32 between buffers of two compiled programs of this context
 * (stream-ordered): hands the KV caches of a prefill plan (token_len = N program) to the decode plan,
 * which the reference does through host-visible program memory. Returns 0 on success. */
int zgml_hip_copy_program_buffer(zgml_hip_ctx* ctx, zgml_hip_program* dst, uint16_t dst_buf, uint64_t dst_offset,
                                 zgml_hip_program* src, uint16_t src_buf, uint64_t src_offset, uint64_t n_elems);
/* KV admission. A lane is the columns of ONE kv head's K or V cache inside a program buffer: f32 columns of d_head floats back to
 * back from f32 element `offset` (block_size 0: a kv head's region of a consolidated cache or of a batched plan's slab), or a whole
 * quantised cache in the layout above (block_size 32, offset 0). The host side lists a plan's lanes per (sequence, layer, kv head,
 * K | V) (DecodeProgram::kv_lanes), so lane i of two plans of one model is the same head. */
typedef struct zgml_kv_lane {
    uint16_t buf, _pad;
    uint32_t d_head, n_cols, block_size; /* block_size 0: f32 columns; 32: the quantised cache layout, offset must be 0 */
    uint64_t offset;                     /* f32 elements to column 0 (f32 lanes) */
} zgml_kv_lane;
/* Columns [src_col, src_col + n) of src lane i -> columns [dst_col, dst_col + n) of dst lane i, i < n_lanes, in ONE launch on the
 * context stream (stream-ordered, non-blocking, like zgml_hip_copy_program_buffer). dst and src may be the same program (fork);
 * a lane pair may not overlap itself. Per lane pair: f32 -> f32 copies the floats; int8 -> int8 copies the column bytes and the
 * column's scales; f32 -> int8 quantises every column as kvq_store does (the bytes and scales are what that op writes for the
 * column, with ONE exception: an exact zero in a block whose largest magnitude is below 127 / FLT_MAX = 3.7e-37 becomes 127, as in
 * the reference, where the device's kvq_store writes -127: zgml_amd/csrc/kvq.h); int8 -> f32 is refused. Admission of a prefill plan's caches into a slot of a batched plan and the fork of a slot
 * are this one call. Returns 0; -1 with an error on the context, before anything is enqueued, for: a dead or elided buffer, a
 * d_head mismatch, columns beyond either n_cols, a lane extent beyond its buffer, a block_size other than 0 / 32 (or d_head % 32
 * on an int8 lane, or an int8 lane with an offset), int8 -> f32, overlapping source and destination ranges of one buffer.
 * n == 0 or n_lanes == 0 does nothing and returns 0. (Moving columns down INSIDE a lane — a context shift — is zgml_hip_kv_shift
 * below: this call refuses a lane pair that overlaps itself and does no arithmetic besides quantisation.) */
int zgml_hip_kv_move(zgml_hip_ctx* ctx, zgml_hip_program* dst, const zgml_kv_lane* dst_lanes, zgml_hip_program* src,
                     const zgml_kv_lane* src_lanes, uint64_t n_lanes, uint32_t src_col, uint32_t dst_col, uint32_t n);
/* Context shift. With n_filled columns of every lane in use, columns [keep + discard, n_filled) of every lane move down to
 * [keep, n_filled - discard), in place, in ONE launch on the context stream (stream-ordered, non-blocking); the first `keep`
 * columns (BOS / system prompt) stay, the next `discard` are dropped, and every other byte of every lane keeps its value, the stale
 * tail [n_filled - discard, n_cols) included. rotate[i] = 1 marks lane i as a K lane: its caches hold keys already turned by RoPE,
 * and every MOVED key is turned back by `discard` positions — pairs (i, i + d_head / 2) as the rope op's, with cos_row[i], sin_row[i]
 * (host, d_head / 2 floats each: the first half of row `discard` of the model's own tables), every product and sum rounded to f32
 * on its own (zgml_amd/csrc/kv_shift.h states the rule; device columns equal it to the bit). An int8 K column is dequantised, turned
 * and requantised as a whole with the column rule of kvq.h — every shift therefore costs an int8 key up to one quantisation unit,
 * shrinking it: shift rarely and by much —; V lanes are copied. Afterwards positions equal column indices again: decoding goes
 * on at position n_filled - discard with the same plan, masks and loops; no forward pass. The shifted cache is NOT a re-prefilled
 * one: kept values and keys still carry the attention of the dropped tokens (llama.cpp's context-shift semantics).
 * All lanes of a call share one d_head. Returns 0; -1 with an error on the context that starts with "kv_shift:", before anything
 * is enqueued, for: every lane check zgml_hip_kv_move makes (dead or elided buffer, block_size, d_head / n_cols 0, extent, int8
 * d_head % 32 and offset), an odd d_head, differing d_head, an int8 K lane whose d_head is neither 32 nor a multiple of 64, d_head > 2048,
 * keep + discard > n_filled, n_filled > n_cols, a NULL row or lane table, two lanes whose extents meet. discard == 0,
 * n_lanes == 0 or keep + discard == n_filled does nothing and returns 0. Not for sharded (zgml_hip_shard_*) programs. */
int zgml_hip_kv_shift(zgml_hip_ctx* ctx, zgml_hip_program* program, const zgml_kv_lane* lanes, const uint8_t* rotate /* [n_lanes]: 1 = a K lane */,
                      uint64_t n_lanes, uint32_t keep, uint32_t discard, uint32_t n_filled,
                      const float* cos_row /* host, d_head / 2 */, const float* sin_row /* host, d_head / 2 */);
/* What one round of the shift's kernel carries (it walks a lane in ascending rounds: kv_shift.hip): values of a K lane, bytes of
 * a V lane. For tests and tools that size a lane to the kernel's loop. */
void zgml_hip_kv_shift_rounds(uint32_t* rotate_values, uint32_t* copy_bytes);
/* Park and resume. zgml_hip_kv_park writes columns [col, col + n) of every lane into the caller's HOST blob: one pack launch into
 * a device staging block the context owns (grown on demand), then one device-to-host copy; it blocks until the blob is complete.
 * zgml_hip_kv_resume writes a blob's n columns into columns [col, col + n) of every lane — any col, not only the park's —: one
 * host-to-device copy into staging, then one unpack launch on the context stream; it returns once the blob has been consumed (the
 * caller may free it) and the launch is stream-ordered like zgml_hip_kv_move. The blob outlives its program: a prompt prefilled
 * once can be handed to any slot of any plan of the same model later (prompt cache), a running sequence can leave its slot and
 * come back (preemption), and an application can keep the bytes (persistence). Token history, penalty window, constraint state
 * and position are the caller's to keep beside it.
 * The blob is self-describing (zgml_amd/csrc/kv_park.h states the layout): a 32-byte header — magic, version, n_lanes, n, flags,
 * total bytes —, a directory of one 16-byte record per lane — d_head, the run's form (f32 | int8), the data offset —, and per lane
 * a data run and, for int8, a scale run of n * d_head / 32 floats, every run on a 16-byte boundary of the blob. The host writes
 * header and directory, the device the payload. zgml_hip_kv_park_bytes is the size of that blob for a lane table; 0 for a table
 * a park would refuse by the records alone.
 * flags bit 0 (ZGML_KV_PARK_INT8): f32 lanes are stored quantised with the column rule of kvq.h (0.28x the bytes at d_head 128);
 * refused for an f32 lane whose d_head % 32 != 0, no effect on int8 lanes. Per lane a resume copies (f32 run -> f32 lane; int8 run
 * -> int8 lane: bytes and scales) or quantises (f32 run -> int8 lane: exactly the bytes zgml_hip_kv_move writes for f32 -> int8);
 * an int8 run into an f32 lane is refused.
 * Both return 0; -1 with an error on the context that starts with "kv_park:" / "kv_resume:", before anything is enqueued, for:
 * every lane check zgml_hip_kv_move makes, columns beyond n_cols, cap below the size, the flag on a lane that cannot take it, a
 * NULL blob or lane table; on resume also a bad magic or version, bytes different from the header's total (or a directory that is
 * not the layout's), n_lanes or a lane's d_head different from the destination's, int8 -> f32, two destination lanes whose
 * written ranges meet. n == 0 or n_lanes == 0 does nothing and returns 0 (a park writes a valid empty blob: the bare header).
 * Not for sharded (zgml_hip_shard_*) programs. */
#define ZGML_KV_PARK_INT8 1u
uint64_t zgml_hip_kv_park_bytes(const zgml_kv_lane* lanes, uint64_t n_lanes, uint32_t n, uint32_t flags);
int zgml_hip_kv_park(zgml_hip_ctx* ctx, zgml_hip_program* program, const zgml_kv_lane* lanes, uint64_t n_lanes, uint32_t col, uint32_t n,
                     uint32_t flags, void* blob, uint64_t cap);
int zgml_hip_kv_resume(zgml_hip_ctx* ctx, zgml_hip_program* program, const zgml_kv_lane* lanes, uint64_t n_lanes, uint32_t col, const void* blob,
                       uint64_t bytes);
/* The HIP stream (hipStream_t as void*) the context launches on. */
void* zgml_hip_stream(zgml_hip_ctx* ctx);
/* Execute without host I/O and without blocking: enqueue the program on the context stream. */
void zgml_hip_enqueue_program(zgml_hip_ctx* ctx, zgml_hip_program* handle);
/* Enqueue ops [first, first+count) only (multi-GPU harness interleaves collectives). */
void zgml_hip_enqueue_ops(zgml_hip_ctx* ctx, zgml_hip_program* handle, uint64_t first, uint64_t count);
/* Declare op indices that batched launches must not straddle (the positions of the harness's
 * collectives); enqueue_ops ranges must start/end on them. */
int zgml_hip_program_set_barriers(zgml_hip_ctx* ctx, zgml_hip_program* handle, const uint64_t* op_indices,
                                  uint64_t n);
void zgml_hip_synchronize(zgml_hip_ctx* ctx);
/* Capture-friendly split of a step, for harnesses that record ops + collectives into ONE graph per
 * token (multi-GPU): stage_inputs does the host side (validation + copy into pinned staging),
 * enqueue_staged the device side (one H2D, scatter kernel, dynamic-parameter block) and may be recorded
 * into a stream capture; a replay picks up what stage_inputs / refresh_program wrote last.
 * enqueue_argmax leaves the index in pinned memory: read it with argmax_result after the stream (or
 * the graph replay) has completed. */
int zgml_hip_stage_inputs(zgml_hip_ctx* ctx, zgml_hip_program* handle, const zgml_program_io* inputs, uint64_t n_inputs);
void zgml_hip_enqueue_staged(zgml_hip_ctx* ctx, zgml_hip_program* handle);
int zgml_hip_enqueue_argmax(zgml_hip_ctx* ctx, zgml_hip_program* handle, uint16_t buf_idx, uint64_t offset, uint64_t n);
int64_t zgml_hip_argmax_result(zgml_hip_ctx* ctx);
/* The two halves of execute_program on their own, for harnesses that interleave collectives with
 * op ranges: enqueue the host->device transfers / run the device->host transfers (blocking). */
void zgml_hip_upload_inputs(zgml_hip_ctx* ctx, zgml_hip_program* handle, const zgml_program_io* inputs,
                            uint64_t n_inputs);
void zgml_hip_download_outputs(zgml_hip_ctx* ctx, zgml_hip_program* handle, const zgml_program_io* outputs,
                               uint64_t n_outputs);
/* On-device greedy argmax over f32 elements [offset, offset+n) of a program buffer: first index
 * of the maximum (strict >), as scripts/generate_llama.zig:101-110 / src/nn.zig:122-138. */
int64_t zgml_hip_argmax(zgml_hip_ctx* ctx, zgml_hip_program* handle, uint16_t buf_idx,
                        uint64_t offset, uint64_t n);

/* ── Row-shard (N-split) execution across the GPUs of one node (the reference has no distributed code) ──
 * One process and one context per GPU. Every quantized weight of the per-rank program is split along N (whole 32-column
 * scale blocks), activations are replicated, KV caches are head-sharded; between op ranges the replicated activation is
 * restored by ONE in-place all-gather (RCCL over xGMI, enqueued on the context stream). librccl.so is opened at run time
 * by these entry points only. Typical use (the host side of zgml_amd/host builds the per-rank program and its gather
 * points): rank 0 calls shard_unique_id and hands the 128 bytes to the other ranks by any channel; every rank calls
 * shard_init, compile_program, shard_attach, then per token refresh_program + shard_step. */
typedef struct zgml_shard_point {
    uint64_t op_end;       /* ops [previous op_end, op_end) run before this gather */
    uint16_t buf_idx;      /* program buffer holding the replicated vector */
    uint16_t _pad;
    uint32_t offset;       /* f32 elements: the vector is [offset, offset + world * len_per_rank) */
    uint32_t len_per_rank; /* rank r owns [offset + r * len_per_rank, ...) before the gather */
} zgml_shard_point;
int zgml_hip_shard_unique_id(unsigned char id_out[128]);                 /* ncclGetUniqueId; 0 on success */
int zgml_hip_shard_init(zgml_hip_ctx* ctx, const unsigned char id[128], int rank, int world); /* ncclCommInitRank on the context's device */
void zgml_hip_shard_destroy(zgml_hip_ctx* ctx);                            /* also done by zgml_hip_destroy */
/* Declare the program's all-gather points (ascending op_end) and the logits the greedy token is taken from
 * (after the last gather every rank holds the full vocabulary). Also sets the plan barriers at those op indices. */
int zgml_hip_shard_attach(zgml_hip_ctx* ctx, zgml_hip_program* program, const zgml_shard_point* points, uint64_t n_points,
                          uint16_t logits_buf, uint64_t vocab);
/* One decode step on this rank: stage + upload the inputs, run the op ranges with the all-gathers between them, argmax
 * of the gathered logits; blocking. The device side is recorded into one graph on the first call and replayed
 * afterwards (ZGML_SHARD_GRAPH=0 or a failed capture: issued eagerly). Returns the greedy token, < 0 on error. Every
 * rank must call it for every step (the collectives are collective). */
int64_t zgml_hip_shard_step(zgml_hip_ctx* ctx, zgml_hip_program* program, const zgml_program_io* inputs, uint64_t n_inputs);
int zgml_hip_shard_step_mode(zgml_hip_program* program); /* 1: steps replay one graph per token, 0: eager */
/* The greedy token of the N-sharded LM head: when the LAST gather point covers the logits buffer, that gather is replaced by
 * one (max, index) pair per rank (8 bytes instead of 4 * vocab / world; first maximum wins, src/nn.zig:122-138) in BOTH gather
 * modes; the logits buffer then holds only the rank's own slice after a step.
 *
 * PEER gather mode (no RCCL; zgml_amd/csrc/shard_peer.hip): every gather point is one small kernel per rank that stores the
 * rank's slice into a staging area in every peer's fine-grained block (xGMI peer stores), counts an arrival on every peer,
 * waits (bounded) for its own arrivals and lands the peers' slices in its program buffer. Use: every rank calls
 * shard_init_peer instead of shard_unique_id / shard_init, then compile_program + shard_attach as before, then exports its
 * block's handle, hands it to every other rank by any channel (64 + 24 bytes), imports the others', and steps as before.
 * Ranks may be processes (hipIpc handles) or contexts of ONE process (raw pointers: how the single-GPU tests run two ranks).
 * A wait that gives up (ZGML_SHARD_PEER_WAIT_MS, default 5000) makes shard_step return -1 with an error on the context. */
typedef struct zgml_shard_peer_handle {
    unsigned char ipc[64]; /* hipIpcMemHandle_t of the block */
    uint64_t pid;          /* exporting process: an importer in the same process uses `raw` */
    uint64_t raw;          /* the block's device pointer in the exporting process */
    uint64_t bytes;
} zgml_shard_peer_handle;
int zgml_hip_shard_init_peer(zgml_hip_ctx* ctx, int rank, int world);
int zgml_hip_shard_peer_export(zgml_hip_ctx* ctx, zgml_hip_program* program, zgml_shard_peer_handle* out);
int zgml_hip_shard_peer_import(zgml_hip_ctx* ctx, zgml_hip_program* program, int peer_rank, const zgml_shard_peer_handle* handle);
/* Diagnostics: one EAGER step with HIP events around every all-gather — device microseconds of the whole step and of the
 * collectives inside it (launch-bound: eager steps are slower than graph replays; the ratio is what it is for). */
int64_t zgml_hip_shard_profile_step(zgml_hip_ctx* ctx, zgml_hip_program* program, const zgml_program_io* inputs, uint64_t n_inputs,
                                    double* step_us, double* gather_us);
/* ... and, gather point by gather point, the microseconds of the last profiled step (writes min(cap, points) values; returns the
 * number of points). With the device ordinal and the peer-access row below, the first multi-device run can be read from one log. */
uint64_t zgml_hip_shard_last_point_us(zgml_hip_program* program, double* out, uint64_t cap);
/* hipDeviceCanAccessPeer(device, peer) as 0 / 1 (-1: the query failed); touches no context. */
int zgml_hip_device_can_access_peer(int device, int peer);
int zgml_hip_device_count(void);

/* Device-resident greedy decode for LLaMA-shaped programs (measurement protocol: inputs already
 * in HBM when the timed region starts). The reference's per-token host work — embedding-row
 * copy, causal-mask column, RoPE row, KV position / seq_kv patching, logits download + argmax
 * (src/llama_inference.zig:405-466, benchmarks/llama_smollm_bench.zig:290-314,
 * scripts/generate_llama.zig:101-110) — is done by one small device kernel before and one after
 * the program graph, from tables uploaded once; a token costs one graph launch and no host<->
 * device traffic. Results are identical to stepping through execute_program (tests check it). */
typedef struct zgml_resident_llama {
    const float* token_embed; /* host [vocab][d_model], uploaded once */
    const float* cos_table;   /* host [max_seq][d_head] */
    const float* sin_table;   /* host [max_seq][d_head] */
    uint32_t vocab, d_model, max_seq, d_head;
    uint16_t buf_token_input, buf_attn_mask, buf_logits, _pad;
    const uint16_t* buf_rope; /* one packed cos|sin leaf per layer */
    uint32_t n_rope;
    uint32_t _pad2;
} zgml_resident_llama;
int zgml_hip_resident_setup(zgml_hip_ctx* ctx, zgml_hip_program* handle, const zgml_resident_llama* desc);
/* Feed `first_token` at `start_pos`, then the argmax of each step, for n_steps; blocking. Writes
 * the n_steps produced tokens. Returns 0 on success. */
int zgml_hip_resident_decode(zgml_hip_ctx* ctx, zgml_hip_program* handle, uint32_t first_token,
                             uint32_t start_pos, uint32_t n_steps, int64_t* tokens_out);

/* The same for a token_len = T plan (a prefill chunk: LlamaInferenceSession.prefill, src/llama_inference.zig:474,
 * src/llm/device_prefill.zig): zgml_hip_resident_setup on the T-token program (T is read off token_input's size), then per
 * chunk only the T token ids cross PCIe — the T embedding rows, the T causal-mask columns, the T RoPE rows per layer,
 * the KV store offsets / seq_kv = start_pos + T and the argmax of the last position's logits are produced on the
 * device. Blocking. Returns the greedy next token (< 0 on error); results equal execute_program on host-patched inputs. */
int64_t zgml_hip_resident_prefill(zgml_hip_ctx* ctx, zgml_hip_program* handle, const uint32_t* tokens, uint32_t n_tokens,
                                  uint32_t start_pos);

/* ── Batched decode: one program step advances n_seqs independent sequences (the host side builds such a program with
 * build_batch_decode_program, zgml_amd/host/llama_decode.hpp: activations [d, B], per-sequence KV slabs, one decode-shaped
 * attention section per sequence). Every dynamic op (KV store offset, attention seq_kv) then follows the position of ITS
 * sequence; set_sequences declares which, once, after compile_program. Every op with a position-dependent field must be
 * listed (n_seqs <= 32, dyn_op_seq[i] < n_seqs), otherwise the call fails with an error on the context. */
int zgml_hip_program_set_sequences(zgml_hip_ctx* ctx, zgml_hip_program* handle, uint32_t n_seqs, const uint32_t* dyn_op_indices,
                                   const uint32_t* dyn_op_seq, uint64_t n_dyn);
/* zgml_hip_refresh_dynamic per sequence: slice_pos[b] / seq_kv[b] (n_seqs entries each) for the ops of sequence b. Same bounds
 * check and the same fall-back to program order as refresh_program. Returns 0, or -1 when no sequences are declared. */
int zgml_hip_refresh_dynamic_batch(zgml_hip_ctx* ctx, zgml_hip_program* handle, const uint32_t* slice_pos, const uint32_t* seq_kv);
/* The device-resident greedy loop over a batched program (zgml_hip_resident_setup on a program with sequences declared reads
 * the T columns of token_input as n_seqs sequences, not T consecutive positions): sequence b starts with first_tokens[b] at
 * start_pos[b] and produces n_steps[b] <= max_steps tokens, written to tokens_out[b * max_steps + i]. A sequence that has
 * produced its count is frozen — same token, same position: its later steps recompute and rewrite the same KV column with the
 * same values — and the rest of its row of tokens_out stays -1. Blocking; one graph launch per step; max(n_steps) steps run.
 * Out-of-range tokens or positions are refused before anything is enqueued. zgml_hip_resident_decode / _prefill refuse a
 * batched program, this call a plain one. Returns 0 on success. */
int zgml_hip_resident_decode_batch(zgml_hip_ctx* ctx, zgml_hip_program* handle, const uint32_t* first_tokens, const uint32_t* start_pos,
                                   const uint32_t* n_steps, uint32_t max_steps, int64_t* tokens_out /* [n_seqs][max_steps] */);

/* ── Greedy-exact speculative decode of ONE sequence on a token_len = T >= 2 plan (zgml_hip_resident_setup on it first).
 * A verify step at (tok, pos) — tok the last confirmed token, not yet in the KV cache — runs the plan over the candidates
 * c[0] = tok, c[j] = the draft for position pos + j (a position without a draft repeats c[j - 1]), exactly as
 * zgml_hip_resident_prefill would at start_pos = pos. With g[j] the first maximum of logits row j, the step accepts the longest
 * prefix c[1..a] with c[j] == g[j - 1], emits g[0..a] (cut to the tokens still wanted) and advances by as many positions. Every
 * emitted token is the greedy token of the plan's own logits over a confirmed context: drafts change how many steps are needed,
 * never which tokens come out. KV columns written for rejected candidates lie at or behind the new position and are stored
 * again by the next step before any attention reads them. After the call the caches are valid for positions
 * < start_pos + n_tokens and unspecified behind that; continue with first_token = tokens_out[n_tokens - 1] at
 * start_pos + n_tokens and the history extended by first_token and tokens_out[0 .. n_tokens - 2].
 * Drafts: mode 0 looks the history's last n tokens up in the history itself (n = ngram down to 1, the latest earlier
 * occurrence of the first n that has one) and proposes what followed it, continuing periodically through its own drafts when the
 * match overlaps the end; mode 1 reads drafts[i] = the caller's guess for the token at position start_pos + 1 + i (an external
 * draft model). Everything runs on the device, one graph launch per step; the host launches ceil(remaining / T) steps, reads
 * the produced count back and repeats until n_tokens are there. */
typedef struct zgml_spec_decode {
    const uint32_t* history; /* tokens at positions 0..start_pos-1 (what filled the cache); NULL with n_history = 0: lookup sees only this call's tokens */
    uint32_t n_history;      /* 0 or start_pos */
    uint32_t mode;           /* 0 = n-gram lookup, 1 = provided */
    const uint32_t* drafts;  /* mode 1 */
    uint32_t n_drafts;
    uint32_t ngram;          /* mode 0: longest suffix tried, 1..4 (0 = 2) */
} zgml_spec_decode;
/* steps: verify steps that emitted something; drafted: real drafts among all candidates (pads are not counted); accepted: the
 * candidates accepted, summed over the steps, before the cut to n_tokens and pads included. */
typedef struct zgml_spec_stats {
    uint32_t steps, drafted, accepted, _pad;
} zgml_spec_stats;
/* Blocking. Returns 0 on success. Refused with -1 and an error on the context, before anything is enqueued: a batched or a
 * token_len = 1 plan, any token (first, history, drafts) >= vocab, n_history neither 0 nor start_pos, mode > 1, ngram > 4,
 * start_pos + n_tokens + T - 1 > max_seq (the last step may start at start_pos + n_tokens - 1 and stores T columns).
 * n_tokens = 0 returns 0 and touches nothing. opt = NULL: lookup with ngram 2 and no history. */
int zgml_hip_resident_decode_speculative(zgml_hip_ctx* ctx, zgml_hip_program* handle, uint32_t first_token, uint32_t start_pos,
                                         uint32_t n_tokens, const zgml_spec_decode* opt, int64_t* tokens_out /* [n_tokens] */,
                                         zgml_spec_stats* stats /* may be NULL */);

/* ── Speculative decode under batching: n_seqs sequences on a batched plan with T = tokens_per_seq >= 2 columns per sequence
 * (build_batch_decode_program's tokens_per_seq; zgml_hip_program_set_sequences, then zgml_hip_resident_setup, which accepts a
 * token_input of n_seqs * T columns: column b * T + j is candidate j of sequence b). Sequence b runs the loop of
 * zgml_hip_resident_decode_speculative (same candidates, same acceptance rule, same emission: zgml_amd/csrc/spec.h) from
 * first_tokens[b] at start_pos[b] until it has n_tokens[b] <= max_tokens tokens, with per_seq[b] (per_seq NULL: every sequence
 * looks up with ngram 2 and no history; else an entry with the fields of the single-sequence call: its own history, mode,
 * drafts, ngram). tokens_out[b * max_tokens + i]; the rest of a row stays -1. stats[b] (stats may be NULL) are sequence b's own.
 * Exactness. Every emitted token of sequence b is the first maximum of the plan's own logits row over b's confirmed context:
 *   drafts decide how many steps run, never which tokens come out, and the other sequences of the batch change neither a
 *   sequence's tokens nor its statistics.
 * Resuming. After the call b's caches are valid for positions < start_pos[b] + n_tokens[b] and unspecified behind that; two
 *   calls give the stream of one: continue with first_token = tokens_out[b][n_tokens[b] - 1] at start_pos[b] + n_tokens[b] and
 *   the history extended by first_tokens[b] and tokens_out[b][0 .. n_tokens[b] - 2].
 * Idling. A sequence that has its count idles: its steps emit nothing and change neither its state, its history nor its
 *   counters, but they still run its last confirmed token T times from its end position and store T KV columns there (the
 *   "unspecified" columns). Hence the bound start_pos[b] + n_tokens[b] + T <= max_seq for EVERY b — one column stricter than the
 *   single-sequence call: the host cannot know which sequence finishes first. n_tokens[b] = 0 is allowed and idles from the
 *   start.
 * Launches. One graph launch per step: [draft, n_seqs sequences] [prep, n_seqs * T columns] [plan] [argmax stage 1 over
 *   n_seqs * T rows] [accept + advance, n_seqs sequences] — the launch count of the single-sequence step, a linear chain, and a
 *   graph of its own (other calls on the program invalidate nothing). The host launches max_b ceil(left_b / T) steps, reads the
 *   n_seqs produced counts back and repeats until every sequence is done; a round in which a sequence with tokens left produced
 *   nothing is an error.
 * Refused with -1 and an error on the context, before anything is enqueued: a plain plan or a batched plan with one column per
 *   sequence; a constraint attached to any sequence (zgml_hip_resident_decode_batch_speculative_constrained serves one); per sequence everything zgml_hip_resident_decode_speculative refuses (a
 *   token — first, history, drafts — >= vocab, n_history neither 0 nor start_pos[b], mode > 1, ngram > 4); the bound above;
 *   n_tokens[b] > max_tokens; NULL arrays. All n_tokens zero: returns 0 and touches nothing.
 * zgml_hip_resident_decode_batch and zgml_hip_resident_decode_batch_sampled refuse a plan with more than one column per sequence
 * (this call, zgml_hip_resident_decode_batch_speculative_sampled and _batch_speculative_constrained are the ones that run it); the single-sequence speculative calls keep refusing every batched plan. Blocking. */
int zgml_hip_resident_decode_batch_speculative(zgml_hip_ctx* ctx, zgml_hip_program* handle, const uint32_t* first_tokens,
                                               const uint32_t* start_pos, const uint32_t* n_tokens, uint32_t max_tokens,
                                               const zgml_spec_decode* per_seq /* [n_seqs] or NULL */,
                                               int64_t* tokens_out /* [n_seqs][max_tokens] */, zgml_spec_stats* stats /* [n_seqs] or NULL */);

/* ── Seeded top-k / top-p sampling: the token tail of the resident loops with a sampled pick instead of the first maximum.
 * The rule is written once, in zgml_amd/csrc/sample.h (the kernels and the CPU tests call the same functions):
 *   candidates: the k = min(top_k, n) largest logits, value descending, the lower index first among equals (-0 == +0, a NaN
 *     counts as -inf). The set never exceeds the 256 largest logits, also when top_p alone would admit more: the one deliberate
 *     deviation from textbook nucleus sampling;
 *   pick: sequential f32 over the candidates: p_j = exp((v_j - v_0) / temperature), top_p < 1 cuts to the smallest prefix whose
 *     sum reaches top_p of the total, the token is the first whose running sum exceeds u times the kept sum;
 *   u: Philox4x32-10, key = seed, counter = (position whose logits are sampled, stream, 0, 0); u = (word 0 >> 8) / 2^24.
 * u depends on (seed, stream, position) alone, so a generation is the same in one call or several, alone or inside a batch, and
 * a device pick equals the header's pick over the same logits to the bit. top_k = 1 is the greedy token.
 * Speculative decode samples through zgml_hip_resident_decode_speculative_sampled (one sequence) and
 * zgml_hip_resident_decode_batch_speculative_sampled (every sequence of a batched plan with its own parameter set), both below;
 * only sharded decode (zgml_hip_shard_step) stays greedy. */
typedef struct zgml_sampling {
    float temperature;   /* > 0 */
    float top_p;         /* (0, 1]; >= 1: no nucleus cut */
    uint32_t top_k;      /* 1..256, 0 = 256 */
    uint32_t n_stop;     /* 0..4 */
    uint32_t stop[4];    /* < vocab */
    uint32_t stream;     /* Philox counter word 1 */
    uint32_t logprobs;   /* 0: off; else keep the log-probability of every token of the call (below). The word was padding before */
    uint64_t seed;
    /* the penalties (below); an all-zero tail: off */
    float repeat_penalty;    /* 0 or 1: neutral; else finite and > 0 */
    float presence_penalty;  /* finite; negative values encourage a token */
    float frequency_penalty; /* finite; likewise */
    uint32_t penalty_window; /* W: 0..256 */
    const uint32_t* recent;  /* the tokens before the call (per entry point, below) */
    uint32_t n_recent;
    uint32_t top_logprobs;   /* 0: off; else, with logprobs != 0, also keep that many alternatives per token (below). The word was padding before */
} zgml_sampling;
/* Repetition, presence and frequency penalties (rule: zgml_amd/csrc/sample.h). The pick at position P — over the logits produced
 *   by feeding the token at P — sees the tokens at positions max(lo, P + 1 - W) .. P, lo the first position whose token the call
 *   knows; count(t) is the number of occurrences of token t among them. A logit v of a token with count c > 0 becomes
 *     v1 = v > 0 ? v * (1 / repeat_penalty) : v * repeat_penalty;  v2 = v1 - c * frequency_penalty;  v3 = v2 - presence_penalty
 *   (one rounded f32 operation each; the multiplication by the reciprocal, computed once on the host, where llama.cpp divides is
 *   the one deliberate deviation, in the last bit), every other logit stays as it is to the bit, and the candidates, the pick and
 *   u are those above over the penalised values. The penalties act BEFORE the 256 largest are selected — a penalised token may
 *   leave the candidates, an encouraged one may enter them from any rank — and before the temperature.
 *   They are active iff penalty_window > 0 and at least one penalty is not neutral. Inactive: exactly the launches and the tokens
 *   of a call without the fields. Active: the same number of launches, the select launch in its penalised form; the loops
 *   replay a captured graph of their own, so calls with and without penalties alternate on one program and invalidate nothing.
 * Where the window comes from:
 *   zgml_hip_resident_decode_sampled, _batch_sampled: recent[0, n_recent) are the tokens at positions start_pos - n_recent ..
 *     start_pos - 1; the library adds first_token at start_pos and every token it emits. lo = start_pos - n_recent; only the last
 *     W - 1 entries are read. Each batched sequence has its own through per_seq[b], and sequences with penalties off sit
 *     beside sequences with them on. A sequence frozen by a stop token or by its count adds nothing; continuing it in a later
 *     call with `recent` re-supplied gives the stream of one uninterrupted call.
 *   zgml_hip_sample: recent[0, n_recent) are the tokens at positions position + 1 - n_recent .. position, the last one the token
 *     whose logits these are. The last W entries are read; a token >= n touches no logit and is ignored.
 *   zgml_hip_resident_decode_speculative_sampled: row j's window is read from the call's own device history and the step's
 *     candidates (history up to the position the step runs at, the candidates behind it); lo is the first position the history
 *     knows (0 with opt->history, else start_pos). `recent` must be NULL: the tokens before the call are opt->history.
 * Refused with -1 and an error on the context, before anything is enqueued: a penalty that is not neutral with
 *   penalty_window = 0; penalty_window > 256; a penalty that is not finite, or repeat_penalty < 0; recent = NULL with
 *   n_recent > 0; in the loops a recent token >= vocab and n_recent > start_pos; in the speculative call recent != NULL. */
/* The log-probability of every sampled token: the word `logprobs` (rule: zgml_amd/csrc/sample.h, "THE LOG-PROBABILITY"). 0: exactly
 *   the launches, the graphs and the tokens of a call without it. Not 0: the call also computes, for every token it emits,
 *   log softmax(row)[token] over the logits row the token was picked from — the WHOLE vocabulary and the RAW logits: before the
 *   penalties, before the temperature, whatever top_k / top_p are; the model's own distribution, independent of how the token was
 *   picked (with penalties on, the value of the token the penalised pick chose under the unpenalised row) — and keeps them on the
 *   context for zgml_hip_logprobs_result (below). A device value equals the header's over the same logits bits, to the bit:
 *   sample_exp, sample_log and the order of every sum are part of the rule. Against float64 the error is at most
 *   1e-5 + 2.4e-7 |v_token - max(row)|.
 *   Why a word and a getter, not an output pointer in the structure: the word takes the four bytes of padding between `stream` and
 *   `seed`, so no field moves and the structure keeps its size — arrays of it, and callers built against the earlier header, stay
 *   valid. A caller that never zeroed the structure may have the word set by accident: that costs two launches per step and
 *   changes no result.
 *   Layout of the values, that of the call's tokens_out: zgml_hip_resident_decode_sampled [n_steps]; _batch_sampled
 *   [n_seqs][max_steps], sequences with and without the word side by side (a row of a sequence without it is all NaN);
 *   _speculative_sampled [n_tokens], entry i the value of tokens_out[i] under the row of the verify step that emitted it;
 *   zgml_hip_sample one float for the returned token. Entries of tokens that were not produced — behind a stop token, behind a
 *   sequence's count, behind the cut — are the quiet NaN 0x7FC00000, the analogue of tokens_out's -1. A frozen sequence's later
 *   steps write nothing. top_k = 1 makes every sampled entry point a greedy loop with log-probabilities: the greedy entry points
 *   have no twin.
 *   Cost: two launches more per step ([partial sums: 4096 logits per workgroup] in front of the select, [finish: one wave per
 *   row] behind the pick), in captured graphs of their own — calls with and without the word, with and without penalties,
 *   alternate on one program and invalidate nothing. Refused with the word set: a row of more than 2^20 logits.
 *   Values: a row without an entry above -inf gives -inf; a row holding +inf gives the NaN above; a token whose logit is -inf
 *   (or NaN, which counts as -inf) gives -inf. */
/* The alternatives of every sampled token: the word `top_logprobs` (rule: zgml_amd/csrc/sample.h, "THE ALTERNATIVES"). It is read
 *   ONLY when logprobs != 0. 0: exactly the launches and graphs of a call with `logprobs` alone. a > 0: the call also keeps, for
 *   every token it emits, the a_eff = min(a, 64, vocab) tokens with the largest logits of the row the token was picked from, in
 *   the candidate order (value descending, the lower index first among equals), each with its log-probability under the rule
 *   above: over the RAW row — before the penalties, before the temperature, whatever top_k / top_p are. Entry 0 is the row's first
 *   maximum; a value equals what zgml_hip_logprobs returns for that token over the same row, to the bit. With penalties on, the
 *   pick's own candidates are the penalised ones, so they are NOT these.
 *   The word takes the four bytes of padding behind `n_recent`: no field moves, the structure keeps its size. A value above 64
 *   is read as 64 and not refused: a caller built against the earlier header that set `logprobs` on a structure it never zeroed
 *   must not start to see refusals; at worst it pays for alternatives it never fetches.
 *   Cost: without active penalties none in launches — the finish launch runs in its top form, which merges the heads of the lists
 *   the select launch left in its scratch —; with active penalties one launch more per step, a select over the raw rows (in a
 *   batched call as soon as one sequence has penalties active). The count lives in the device parameter table: one captured
 *   graph per form serves every a >= 1, and calls with and without the word alternate on one program and invalidate nothing.
 *   The values are fetched with zgml_hip_top_logprobs_result (below). */
/* The alternatives that the context's last call with logprobs != 0 and top_logprobs != 0 left behind, as
 *   [entries of that call's tokens_out][width]: width is the largest effective count among the call's sequences (each sequence of
 *   _batch_sampled has its own; one with a smaller count, or none, is padded), entry (i, j) alternative j of tokens_out[i] — in
 *   _speculative_sampled of the row of the verify step that emitted it. Padding, and every entry of a token that was not produced
 *   (behind a stop token, a count, the cut of a speculative step), is token -1 and the quiet NaN 0x7FC00000.
 *   Copies min(n, entries x width) pairs and returns entries x width (0 before any such call); *width_out (may be NULL) receives
 *   width. A later call without the word leaves the values as they are. -1 with an error on the context: an output pointer NULL
 *   with n > 0. */
int64_t zgml_hip_top_logprobs_result(zgml_hip_ctx* ctx, int64_t* tokens_out, float* logprobs_out, uint64_t n, uint32_t* width_out);
/* The values that the context's last call with the `logprobs` word set left behind, in the layout above: copies min(n, their
 * number) floats to out and returns their number (0 before any such call); a call without the word leaves them as they are.
 * -1 with an error on the context: out NULL with n > 0. */
int64_t zgml_hip_logprobs_result(zgml_hip_ctx* ctx, float* out, uint64_t n);
/* The sampling sibling of zgml_hip_argmax over f32 elements [offset, offset + n) of a program buffer, 1 <= n < 2^32; blocking.
 * `position` is the Philox counter's word 0; stop tokens are not looked at. For vtable-path callers, and for the first token
 * after zgml_hip_resident_prefill, whose logits rows stay in the buffer. candidates_out (NULL or 256 words) receives the
 * candidates' indices in order, *n_candidates_out (may be NULL) their number. Returns the token, -1 with an error on the context
 * for parameters out of range (below) or a range outside the buffer. sampling->logprobs (above): one float, the returned token's, for
 * zgml_hip_logprobs_result; with sampling->top_logprobs one row of alternatives for zgml_hip_top_logprobs_result. */
int64_t zgml_hip_sample(zgml_hip_ctx* ctx, zgml_hip_program* handle, uint16_t buf_idx, uint64_t offset, uint64_t n,
                        const zgml_sampling* sampling, uint32_t position, uint32_t* candidates_out /* NULL or [256] */,
                        uint32_t* n_candidates_out);
/* The scoring sibling of zgml_hip_sample: logprobs_out[i] = log softmax(row i)[tokens[i]] (the rule above) over `rows` consecutive
 * rows of n f32 elements each, row i at [offset + i n, offset + (i + 1) n) of a program buffer; blocking; two launches whatever
 * `rows` is. After zgml_hip_resident_prefill of a T-token chunk at start_pos, row i of the logits buffer with tokens[i] = the
 * prompt's token at start_pos + i + 1 is that token's log-likelihood: a prompt is scored with T - 1 floats per chunk coming
 * back instead of T x vocab logits. Returns 0. Refused with -1 and an error on the context, nothing enqueued: n = 0, n > 2^20,
 * rows = 0, a token >= n, a range outside the buffer, tokens or logprobs_out NULL. */
int zgml_hip_logprobs(zgml_hip_ctx* ctx, zgml_hip_program* handle, uint16_t buf_idx, uint64_t offset, uint64_t n, uint32_t rows,
                      const uint32_t* tokens /* [rows] */, float* logprobs_out /* [rows] */);
/* The alternatives sibling of zgml_hip_logprobs: row i's min(top_n, n) largest logits as (token, log-probability) pairs, in the
 * order and under the rule of the `top_logprobs` word above, into tokens_out[i][0 ..] and logprobs_out[i][0 ..]; entries behind
 * min(top_n, n) are -1 and the quiet NaN. Blocking; three launches ([partial] [select] [finish + top]) whatever `rows` is. Returns
 * 0. Refused with -1 and an error on the context, nothing enqueued: everything zgml_hip_logprobs refuses of n, rows, the range and
 * NULL pointers, and top_n outside 1 .. 64 (a new argument: refused, not clamped). */
int zgml_hip_top_logprobs(zgml_hip_ctx* ctx, zgml_hip_program* handle, uint16_t buf_idx, uint64_t offset, uint64_t n, uint32_t rows,
                          uint32_t top_n, int64_t* tokens_out /* [rows][top_n] */, float* logprobs_out /* [rows][top_n] */);
/* zgml_hip_resident_decode with the sampled tail: per token [prep] [plan] [select] [merge + pick + advance], three launches
 * beside the plan's, one graph launch per token. The parameters live in a device table uploaded per call, so one captured graph —
 * a separate one from the greedy loop's: alternating calls on one program invalidate nothing — serves every parameter set.
 * A sequence that emits one of its stop tokens records it and then freezes as a batched sequence that has used up its count
 * does (same token, same position: the remaining steps rewrite the KV column behind the stop token with the same values); the
 * rest of tokens_out is -1 and *n_produced (may be NULL) counts up to and including the stop token. Continue from a stop, or
 * from the end, with first_token = the last token at start_pos + *n_produced.
 * Refused with -1 and an error on the context, before anything is enqueued: temperature not > 0 or top_p not in (0, 1] (a NaN
 * included), top_k > 256, n_stop > 4, a stop token >= vocab, a token_len > 1 or batched plan, and tokens / positions out of range
 * under the rules of zgml_hip_resident_decode. */
int zgml_hip_resident_decode_sampled(zgml_hip_ctx* ctx, zgml_hip_program* handle, uint32_t first_token, uint32_t start_pos,
                                     uint32_t n_steps, const zgml_sampling* sampling, int64_t* tokens_out /* [n_steps] */,
                                     uint32_t* n_produced);
/* zgml_hip_resident_decode_batch with the sampled tail: sequence b samples with per_seq[b] — its own parameters, stream and stop
 * set — and n_produced[b] (the array may be NULL) counts its tokens. A sequence frozen by a stop token does not affect the
 * others. Refusals as above per sequence, and those of zgml_hip_resident_decode_batch; a plain plan is refused. */
int zgml_hip_resident_decode_batch_sampled(zgml_hip_ctx* ctx, zgml_hip_program* handle, const uint32_t* first_tokens, const uint32_t* start_pos,
                                           const uint32_t* n_steps, uint32_t max_steps, const zgml_sampling* per_seq /* [n_seqs] */,
                                           int64_t* tokens_out /* [n_seqs][max_steps] */, uint32_t* n_produced /* [n_seqs] */);

/* ── Sampled speculative decode: zgml_hip_resident_decode_speculative with seeded top-k / top-p picks in the verify step.
 * Verify step. A step at (tok, pos) is that of zgml_hip_resident_decode_speculative with one change: g[j] is the pick of
 *   zgml_amd/csrc/sample.h over logits row j with u from counter word 0 = pos + j — the position whose logits are sampled, the
 *   convention of zgml_hip_resident_decode_sampled. The candidates, the pads, the draft modes, the acceptance rule (the longest
 *   prefix c[1..a] with c[j] == g[j - 1]) and which KV columns are valid afterwards are unchanged. Per step [draft] [prep, T
 *   tokens] [plan] [select over T rows] [merge + pick over T rows] [accept + advance]: one launch more than the greedy step,
 *   one graph launch per step, a graph of its own (greedy and sampled speculative calls and zgml_hip_resident_prefill alternate
 *   on one program and invalidate nothing). All T rows read the one parameter set.
 * Exactness. u depends on (seed, stream, position) alone and the candidate list of a row is one well-defined list, so the token
 *   sampled at a position is a deterministic function of that position's logits bits, exactly as the first maximum is. Every
 *   emitted token is the header's pick over the plan's own logits row over a confirmed context at its own position: drafts change
 *   how many steps run, and by the rule never which tokens come out; a generation is the same in one call or several. This is
 *   NOT stochastic (rejection-sampling) acceptance: that would accept more drafts of a stochastic draft model but make the stream
 *   depend on the drafts; here no draft probabilities exist or are needed.
 *   What "the plan's own logits" are to the bit: a row's logits depend neither on the tokens of the other rows nor on which row
 *   of its step it is, but a KV column stored as a later row of a step and the same column stored as row 0 differ in the last
 *   bit on the device, so how the confirmed context was grouped into steps — which the drafts decide — moves a position's logits
 *   by about 1e-7 of their range. The same drafts give the same stream, always; other drafts give the same stream unless a pick's
 *   u lands within that difference of a cumulative boundary (measured: one token of 256 in one of eight SmolLM-135M
 *   configurations, the streams equal again from the next token; none at Llama-2-7B).
 *   With penalties the argument carries over: row j's token is a deterministic function of its logits bits AND of its window —
 *   the confirmed tokens plus the candidates c[1..j]. If row j is used at all, those candidates were accepted, so they are the
 *   confirmed tokens at their positions: the window of an emitted token never holds a rejected draft.
 *   top_k = 1 (penalties neutral) gives exactly the tokens (and statistics) of zgml_hip_resident_decode_speculative.
 *   Against zgml_hip_resident_decode_sampled on a token_len = 1 plan with the same parameters the stream is the same whenever the
 *   two plans' logits lead to the same picks. The M = T and M = 1 kernels agree to the parity bar only, not to the bit, so a pick
 *   whose u lands within that difference of a cumulative boundary (or whose candidate order turns on a near-tie) may legitimately
 *   differ, and the streams part from there: the sampling analogue of the greedy form's tie condition.
 * Stop tokens (sampling->stop). Among the tokens a step would emit, g[0..m-1] (m after the cut to the tokens still wanted), the
 *   first stop token cuts the emission behind itself: it is recorded and the call is finished. The rest of tokens_out is -1 and
 *   *n_produced (may be NULL) counts up to and including the stop token; without a stop it is n_tokens. stats.accepted counts a
 *   before any cut, as in the greedy form. Continue — from a stop or from the end — with first_token = tokens_out[*n_produced - 1]
 *   at start_pos + *n_produced; the caches are valid for positions < start_pos + *n_produced.
 * Blocking. Returns 0 on success. Refused with -1 and an error on the context, before anything is enqueued: everything
 *   zgml_hip_resident_decode_speculative refuses (a batched or a token_len = 1 plan, any token >= vocab, n_history neither 0 nor
 *   start_pos, mode > 1, ngram > 4, start_pos + n_tokens + T - 1 > max_seq) and everything zgml_hip_resident_decode_sampled
 *   refuses of the parameters (temperature not > 0, top_p not in (0, 1], top_k > 256, n_stop > 4, a stop token >= vocab);
 *   sampling = NULL. n_tokens = 0 returns 0 and touches nothing. opt = NULL: lookup with ngram 2 and no history. */
int zgml_hip_resident_decode_speculative_sampled(zgml_hip_ctx* ctx, zgml_hip_program* handle, uint32_t first_token, uint32_t start_pos,
                                                 uint32_t n_tokens, const zgml_spec_decode* opt, const zgml_sampling* sampling,
                                                 int64_t* tokens_out /* [n_tokens] */, uint32_t* n_produced /* may be NULL */,
                                                 zgml_spec_stats* stats /* may be NULL */);

/* ── Sampled speculative decode under batching: zgml_hip_resident_decode_batch_speculative with seeded picks per sequence.
 * Sequence b of a batched plan with T = tokens_per_seq >= 2 columns per sequence runs exactly the loop of
 * zgml_hip_resident_decode_speculative_sampled with sampling[b] and per_seq[b] (per_seq NULL: every sequence looks up with ngram 2
 * and no history): the same candidates, pads, draft modes and acceptance rule (zgml_amd/csrc/spec.h); g[j] is the pick of
 * zgml_amd/csrc/sample.h over logits row b * T + j with counter word 0 = the run position of b + j. Every sequence has its own
 * parameter set, stream, seed and stop set; sequences with different parameters sit side by side. tokens_out[b * max_tokens + i].
 * Exactness. As in the single-sequence call, per sequence: an emitted token is a deterministic function of its row's logits bits,
 *   its window and (seed, stream, position); the other sequences of the batch change neither a sequence's tokens nor its
 *   statistics. top_k = 1 on every sequence (penalties neutral) gives exactly the tokens and statistics of
 *   zgml_hip_resident_decode_batch_speculative.
 * Idling and the bound are those of zgml_hip_resident_decode_batch_speculative: a sequence that has its count idles at its end
 *   position, start_pos[b] + n_tokens[b] + T <= max_seq for every b, n_tokens[b] = 0 is allowed.
 * Stop tokens (sampling[b].stop). The cut of the single-sequence call, per sequence: the first stop token among the tokens a step
 *   of b would emit is recorded and finishes b, which idles from there while the others go on. n_produced[b] (n_produced may be
 *   NULL) counts up to and including the stop token, the rest of the row is -1, stats[b].accepted counts before any cut. The
 *   host launches max_b ceil((wanted_b - produced_b) / T) steps per round with wanted_b read back from the device, so a stop
 *   shortens the round; a round in which a sequence with tokens left produced nothing is an error.
 * Penalties. Row b * T + j's window is sequence b's device history up to its run position plus its candidates c[1..j]; the first
 *   position known is b's own (0 with a history, else start_pos[b]). sampling[b].recent must be NULL, as in the single-sequence
 *   call (the tokens before the call are per_seq[b].history). Sequences with penalties on and off sit side by side.
 * `logprobs` is per sequence; zgml_hip_logprobs_result hands out [n_seqs][max_tokens] values, entry (b, i) the value of
 *   tokens_out[b][i] under the row of the verify step that emitted it; an entry that was not produced holds the quiet NaN
 *   0x7FC00000, and so does the whole row of a sequence without the word. Cost: two launches more per step, graphs of their own.
 * `top_logprobs` is not kept by this call: the word is ignored, not refused (it was padding before), and
 *   zgml_hip_top_logprobs_result is left as the last call that kept alternatives left it.
 * Launches. One graph launch per step: [draft, n_seqs sequences] [prep, n_seqs * T columns] [plan] [select, grid (slices, T,
 *   n_seqs): n_seqs * T rows] [merge + pick, grid (1, T, n_seqs)] [accept + advance, n_seqs sequences] — one launch more than the greedy
 *   batched step, a linear chain. Graphs of its own, one per form (plain, penalised, each with and without `logprobs`): greedy,
 *   sampled and penalised batched speculative calls alternate on one program and invalidate nothing.
 * Resuming. After the call b's caches are valid for positions < start_pos[b] + n_produced[b]; continue with first_token =
 *   tokens_out[b][n_produced[b] - 1] at start_pos[b] + n_produced[b] and the history extended by first_tokens[b] and the tokens
 *   before that one.
 * Blocking. Returns 0 on success. Refused with -1 and an error on the context that names the sequence, before anything is
 *   enqueued: everything zgml_hip_resident_decode_batch_speculative refuses (a plain plan, one column per sequence, a constraint
 *   attached to any sequence — zgml_hip_resident_decode_batch_speculative_constrained serves those —, the per-sequence requests, the bound,
 *   n_tokens[b] > max_tokens, NULL arrays); per sequence everything zgml_hip_resident_decode_speculative_sampled refuses of the
 *   parameters, recent != NULL included; sampling = NULL. All n_tokens zero: returns 0 and touches nothing on the device. */
int zgml_hip_resident_decode_batch_speculative_sampled(zgml_hip_ctx* ctx, zgml_hip_program* handle, const uint32_t* first_tokens,
                                                       const uint32_t* start_pos, const uint32_t* n_tokens, uint32_t max_tokens,
                                                       const zgml_spec_decode* per_seq /* [n_seqs] or NULL */,
                                                       const zgml_sampling* sampling /* [n_seqs], never NULL */,
                                                       int64_t* tokens_out /* [n_seqs][max_tokens] */,
                                                       uint32_t* n_produced /* [n_seqs] or NULL */,
                                                       zgml_spec_stats* stats /* [n_seqs] or NULL */);

/* ── Constrained decoding: a token automaton masks the sampled picks on the device (rule: zgml_amd/csrc/sample.h, THE CONSTRAINT).
 * The caller brings the table, in class-compressed form: class_of[i] is the class of token i, next[s][c] the state behind a
 * token of class c in state s, 0xFFFF where such a token is not allowed in s. There is no grammar compiler here and no additive
 * logit bias.
 * Rule. A token that is not allowed in the sequence's current state is no candidate at all: the candidates are the
 *   min(top_k, number of allowed tokens) largest logits among the allowed ones, the pick and its random number are unchanged, and
 *   penalties apply to the allowed tokens as ever. top_k = 1 is constrained greedy decoding. Behind every pick the state becomes
 *   next[state][class_of[token]]; a stop token advances it too. The state lives on the device and persists across calls: two
 *   calls give the stream of one. A state that allows no token produces nothing: in the loops the sequence freezes as behind a
 *   stop token (tokens_out keeps -1, *n_produced does not count a token, the state stays); zgml_hip_sample returns -1 with an
 *   error on the context. Log-probabilities and alternatives (`logprobs`, `top_logprobs`) are over the RAW row, unaffected by the
 *   constraint exactly as they are unaffected by penalties.
 * Who honours it. zgml_hip_resident_decode_sampled and _batch_sampled: every batched sequence has its own automaton and state,
 *   sequences with and without one side by side; a constrained call replays graphs of its own, so calls with and without a
 *   constraint alternate on one program and invalidate nothing, and a call without one launches exactly what it launched before.
 *   zgml_hip_sample honours it when n equals the automaton's vocab: it uses sequence 0's state and advances it over the returned
 *   token (resident prefill, zgml_hip_sample for the first token, then the sampled loop: no host bookkeeping), and
 *   candidates_out receives the constrained candidates. zgml_hip_resident_prefill is unchanged: the greedy token it returns is
 *   unconstrained.
 *   zgml_hip_resident_decode_speculative_constrained (below) honours sequence 0's in the verify step of a token_len = T plan,
 *   zgml_hip_resident_decode_batch_speculative_constrained (below) every sequence's own in the verify step of a batched plan with
 *   tokens_per_seq >= 2, zgml_hip_resident_decode_speculative_model_constrained (below) the TARGET's sequence 0's in the drafts
 *   of a draft model and in the verify step.
 * Refused. While any constraint is attached to the program, zgml_hip_resident_decode, zgml_hip_resident_decode_batch,
 *   zgml_hip_resident_decode_speculative, zgml_hip_resident_decode_speculative_sampled, zgml_hip_resident_decode_batch_speculative,
 *   zgml_hip_resident_decode_batch_speculative_sampled, zgml_hip_resident_decode_speculative_model and zgml_hip_resident_decode_batch_speculative_model (a constraint on
 *   the target or on the draft; zgml_hip_resident_decode_speculative_model_constrained serves one on the target of a single sequence) and zgml_hip_shard_step return -1 with an error on the context and enqueue nothing: they would pick tokens while ignoring the
 *   constraint. */
typedef struct zgml_token_dfa {
    uint32_t n_states, n_classes, vocab, _pad; /* 1 <= n_states <= 65535, 1 <= n_classes <= 8192 */
    const uint16_t* class_of;                  /* [vocab], every entry < n_classes */
    const uint16_t* next;                      /* [n_states][n_classes], 0xFFFF: not allowed, else < n_states */
} zgml_token_dfa;
typedef struct zgml_hip_constraint zgml_hip_constraint;
/* Validates the automaton and uploads it once; it may then be attached to any number of sequences of any programs of the
 * context. NULL with an error on the context, before anything is uploaded: a NULL table, sizes outside the limits, a class
 * >= n_classes, a next state >= n_states that is not 0xFFFF. */
zgml_hip_constraint* zgml_hip_constraint_create(zgml_hip_ctx* ctx, const zgml_token_dfa* dfa);
/* Frees it; a constraint that is still attached to a sequence is refused (an error on the context, nothing freed): detach first.
 * Freeing a program, or setting it up again, detaches its sequences. */
void zgml_hip_constraint_free(zgml_hip_ctx* ctx, zgml_hip_constraint* constraint);
/* Attaches `constraint` to sequence `seq` of a program after zgml_hip_resident_setup (seq 0 of a plain plan) with the sequence's
 * state set to `state`; constraint = NULL detaches (state is ignored). Blocking. Returns 0; -1 with an error on the context
 * and nothing changed: no resident set-up, seq >= the number of sequences, a vocab different from the program's,
 * state >= n_states. */
int zgml_hip_program_set_constraint(zgml_hip_ctx* ctx, zgml_hip_program* handle, uint32_t seq, zgml_hip_constraint* constraint, uint32_t state);
/* The sequence's current state (a blocking read); -1: none attached (or seq out of range, no resident set-up). */
int64_t zgml_hip_program_constraint_state(zgml_hip_ctx* ctx, zgml_hip_program* handle, uint32_t seq);

/* ── Constrained speculative decode: zgml_hip_resident_decode_speculative_sampled whose verify rows walk the token automaton
 * attached to sequence 0 (rule: zgml_amd/csrc/spec.h, UNDER A CONSTRAINT, and sample.h). With no constraint attached the call IS
 * zgml_hip_resident_decode_speculative_sampled: same tokens, same launches, same graphs. top_k = 1 is constrained greedy
 * speculation.
 * Forced tokens. zgml_hip_constraint_create also computes forced[state]: the single token the state allows when it allows
 *   exactly one token of the vocabulary (a class without tokens counts as nothing), none otherwise. A forced token needs no draft
 *   and cannot be rejected: a step inside a run of forced tokens emits T tokens whatever the logits say ("jump-forward").
 * Candidates. c[0..T-1] and the count of real drafts come from the draft mode as ever. Then one pass runs from s = the sequence's
 *   state, row_state[0] = s; for j = 1 .. T-1: s dead -> row j is dead and c[j] stays; else forced[s] exists -> c[j] = forced[s],
 *   also over a real draft (a different draft is certainly wrong); else j behind the real drafts -> the pad is re-evaluated,
 *   c[j] = c[j - 1]; then s = next[s][class_of[c[j]]], dead when c[j] is not allowed in s, and row_state[j] = s. stats.drafted
 *   grows by the mode's real drafts plus the forced tokens placed at pad positions.
 * Picks. g[j] is the constrained pick (above) of logits row j under row_state[j], u from counter word 0 = pos + j, its penalty
 *   window that of the sampled verify step. A dead row has no candidates; a row without candidates has no pick (internally the
 *   sentinel 0xFFFFFFFF, which equals no candidate).
 * Acceptance, emission, state. The acceptance rule is unchanged; a row without a pick matches nothing, so a dead row is never
 *   reached through accepted candidates. When g[a] has no pick, the reached state allows no token: g[0..a-1] are emitted (possibly
 *   nothing) and the call is finished as behind a stop token — it returns 0, *n_produced counts what came out, the rest of
 *   tokens_out is -1. Stop tokens cut as in the sampled form, and a stop token advances the state too. The sequence's state word
 *   then advances over exactly the emitted tokens; it persists across calls (two calls give the stream of one;
 *   zgml_hip_program_constraint_state reads it).
 * Exactness. The contract of the sampled form: every emitted token is the constrained pick over the plan's own logits row, over a
 *   confirmed context, at its own position and state. Drafts and forced tokens change how many steps run, never which tokens
 *   come out.
 * Log-probabilities and alternatives are over the RAW row, unaffected by the constraint; entries behind *n_produced are the quiet
 *   NaN and -1.
 * Launches. Those of the sampled verify step — [draft] [prep] [plan] [select] [merge + pick] ([log-probability launches])
 *   [accept] —: the constraint adds none. Graphs of its own: constrained calls, plain sampled speculative calls (detached) and
 *   zgml_hip_resident_prefill alternate on one program and invalidate nothing.
 * Refused with -1 and an error on the context, before anything is enqueued: everything
 *   zgml_hip_resident_decode_speculative_sampled refuses, sampling->recent != NULL included. */
int zgml_hip_resident_decode_speculative_constrained(zgml_hip_ctx* ctx, zgml_hip_program* handle, uint32_t first_token, uint32_t start_pos,
                                                     uint32_t n_tokens, const zgml_spec_decode* opt, const zgml_sampling* sampling,
                                                     int64_t* tokens_out /* [n_tokens] */, uint32_t* n_produced /* may be NULL */,
                                                     zgml_spec_stats* stats /* may be NULL */);

/* ── Constrained speculative decode under batching: zgml_hip_resident_decode_batch_speculative_sampled whose verify rows walk the
 * token automata attached to the sequences. Sequence b of a batched plan with T = tokens_per_seq >= 2 columns per sequence runs
 * exactly the loop of zgml_hip_resident_decode_speculative_constrained with sampling[b], per_seq[b] and the automaton and state
 * attached to it through zgml_hip_program_set_constraint(.., seq = b, ..). Every sequence may have its own automaton — class
 * counts and state counts may differ —, and sequences with and without one sit side by side. With no constraint attached to any
 * sequence the call IS zgml_hip_resident_decode_batch_speculative_sampled: same tokens, same launches, same graphs.
 * Rule. No new one (zgml_amd/csrc/spec.h, UNDER A CONSTRAINT, and sample.h): per attached sequence the pass over its candidates
 *   from its state — forced tokens placed, pads re-evaluated, row_state[b * T + j] —, the constrained pick of logits row b * T + j
 *   under that row's state with sampling[b], u from counter word 0 = the run position of b + j, the dead-end cut, and the advance
 *   of b's state word over exactly the tokens b emitted, a stop token included.
 * A sequence without an automaton behaves exactly as in zgml_hip_resident_decode_batch_speculative_sampled: the pass leaves its
 *   candidates alone, none of its rows is dead, its picks are unmasked, and stats[b].drafted grows by its mode's real drafts alone.
 * Dead end. A reached state of b without tokens finishes b as a stop token does: n_produced[b] counts what came out (possibly
 *   nothing), the rest of its row is -1, its state stays; b idles from there, the other sequences go on, and the call returns 0
 *   with no error on the context. The host's round loop reads b's wanted word back before it judges a round: a sequence whose
 *   device words say wanted == produced is finished, not failed.
 * Exactness. Per sequence the contract of the single-sequence call; the other sequences of the batch — their automata, drafts and
 *   parameters — change neither a sequence's tokens nor its statistics nor its state.
 * Idling, the bound start_pos[b] + n_tokens[b] + T <= max_seq, resuming (two calls give the stream and the state of one), stop
 *   tokens, penalties (sampling[b].recent must be NULL) and `logprobs` (over the RAW row, unaffected by the mask; the quiet NaN
 *   behind n_produced[b] and in the whole row of a sequence without the word) are those of
 *   zgml_hip_resident_decode_batch_speculative_sampled. `top_logprobs` stays ignored, as there.
 * Launches. One graph launch per step, no launch more than the sampled batched step: [draft, n_seqs sequences] [prep, n_seqs * T
 *   columns] [plan] [select, grid (slices, T, n_seqs)] [merge + pick, grid (1, T, n_seqs)] ([log-probability launches]) [accept +
 *   advance, n_seqs sequences]. The one select serves rows with and without penalties, with and without an automaton. Graphs of
 *   its own (with and without `logprobs`): constrained calls, detached sampled calls and greedy batched speculative calls
 *   alternate on one program and invalidate nothing.
 * Blocking. Returns 0 on success. Refused with -1 and an error on the context, before anything is enqueued: everything
 *   zgml_hip_resident_decode_batch_speculative_sampled refuses except the attached constraint. */
int zgml_hip_resident_decode_batch_speculative_constrained(zgml_hip_ctx* ctx, zgml_hip_program* handle, const uint32_t* first_tokens,
                                                           const uint32_t* start_pos, const uint32_t* n_tokens, uint32_t max_tokens,
                                                           const zgml_spec_decode* per_seq /* [n_seqs] or NULL */,
                                                           const zgml_sampling* sampling /* [n_seqs], never NULL */,
                                                           int64_t* tokens_out /* [n_seqs][max_tokens] */,
                                                           uint32_t* n_produced /* [n_seqs] or NULL */,
                                                           zgml_spec_stats* stats /* [n_seqs] or NULL */);

/* ── Speculative decode with a draft model: a second resident program drafts for the target (rule: zgml_amd/csrc/spec.h, DRAFTS
 * FROM A MODEL). A sibling of zgml_hip_resident_decode_speculative and _speculative_sampled, not a mode of them: zgml_spec_decode
 * keeps its layout and those calls keep refusing mode > 1.
 * Programs. `target` is a plain token_len = T >= 2 plan with a resident set-up, as for zgml_hip_resident_decode_speculative;
 *   `draft` a plain token_len = 1 plan of the same context with a resident set-up of its own and the target's vocabulary — every
 *   other dimension, the weight kind and the KV form (f32 or int8) may differ.
 * Verify step at (hist[pos], pos). c[0] = hist[pos]; for j = 0 .. T-1 the draft executes on c[j] at position pos + j, storing its
 *   own KV column pos + j; d[j] is the first maximum of its logits row and c[j + 1] = d[j] for j < T - 1. The T-th execution
 *   exists for its KV column alone (after full acceptance the next step starts at pos + T). Then the target's verify step runs
 *   over c[0..T-1] as ever: acceptance, emission and the cuts are those of the sibling calls. stats.drafted grows by T - 1 per
 *   step that emits something; there are no pads. The drafts are the draft's GREEDY tokens, also under a sampled verify step.
 *   Idle steps (a round already launched, nothing left to produce) execute the draft T times from the token and position the
 *   target idles at: that column is rewritten with the same values, the columns behind it are unspecified for both programs.
 * sampling = NULL: the greedy verify step (first maxima; *n_produced = n_tokens). Else the step of
 *   zgml_hip_resident_decode_speculative_sampled, all of it, from the target's rows: picks, stop tokens, penalties over the call's
 *   device history, `logprobs`, `top_logprobs` and the result getters; sampling->recent must be NULL. top_k = 1 with neutral
 *   penalties gives the tokens and statistics of the greedy form.
 * Caches. On entry both programs' caches are valid for positions < start_pos — fill the draft's as the target's: vtable steps, a
 *   prefill plan, zgml_hip_kv_move —; on return both are valid for positions < start_pos + *n_produced. Two calls give the token
 *   stream of one; the second call's statistics are those of a fresh call from that state.
 * Exactness. The contract of the sibling calls: every emitted token is the target's own greedy token (or pick) over a confirmed
 *   context. Drafts decide how many steps run, never which tokens come out.
 * Launches. One graph launch per step, a linear chain: [draft launch] T x { [draft prep] [draft plan] [argmax stage 1] [stage 2 +
 *   draft advance] } [prep, T columns] [target plan] [argmax stage 1 over T rows | the sampled tail] [accept]. The draft
 *   executions use the plain form (not the streaming head of zgml_hip_resident_decode). The graphs belong to the (target, draft)
 *   pair, one per form, apart from every other graph: other calls on either program alternate with this one and invalidate
 *   nothing; another draft program — or the same one freed, set up again or rebuilt, also a new program at its old address —
 *   re-captures. Runtime profile: the target counts plan + 3 + tail launches per step, the draft T x (plan + 3).
 * Blocking. Returns 0. Refused with -1 and an error on the context, before anything is enqueued: everything
 *   zgml_hip_resident_decode_speculative refuses of the target and of the request (history / n_history as its opt->history), with
 *   `sampling` everything _speculative_sampled refuses; a sharded target; a draft that is NULL, without a resident set-up, of
 *   another context, batched, token_len != 1, sharded, the target itself, or of another vocabulary;
 *   start_pos + n_tokens + T - 1 > the draft's max_seq; a constraint attached to either program (a draft model under the
 *   target's constraint is zgml_hip_resident_decode_speculative_model_constrained, below; a draft model under batching is
 *   zgml_hip_resident_decode_batch_speculative_model). n_tokens = 0 returns 0 and touches nothing. */
int zgml_hip_resident_decode_speculative_model(zgml_hip_ctx* ctx, zgml_hip_program* target, zgml_hip_program* draft, uint32_t first_token,
                                               uint32_t start_pos, uint32_t n_tokens, const uint32_t* history /* [n_history] */,
                                               uint32_t n_history /* 0 or start_pos */, const zgml_sampling* sampling /* NULL: greedy */,
                                               int64_t* tokens_out /* [n_tokens] */, uint32_t* n_produced /* may be NULL */,
                                               zgml_spec_stats* stats /* may be NULL */);

/* ── Speculative decode with a draft model under a constraint: the draft is masked (rule: zgml_amd/csrc/spec.h, DRAFTS FROM A
 * MODEL UNDER A CONSTRAINT). A sibling of zgml_hip_resident_decode_speculative_model, not a mode of it: that call keeps refusing
 * an attached constraint. The constraint is the one attached to the TARGET (zgml_hip_program_set_constraint, sequence 0); the
 * programs are those of zgml_hip_resident_decode_speculative_model.
 * Verify step at (hist[pos], pos). c[0] = hist[pos], row_state[0] = the sequence's state. For j = 0 .. T-1 the draft executes on
 *   c[j] at position pos + j and stores its own KV column. For j < T - 1, with s = row_state[j]: s dead, or s allows no token ->
 *   there is no draft, c[j + 1] = c[j] and row j + 1 is dead; otherwise c[j + 1] = the first maximum of the draft's logits row
 *   over the tokens allowed in s (larger value wins, lower index among equals; a forbidden token is no candidate at all, so the
 *   first allowed token wins over a row of -inf) and row_state[j + 1] = next[s][class_of[c[j + 1]]], never dead. In a state that
 *   forces a token the masked maximum is that token whatever the logits say: forced runs are drafted without a placing pass.
 *   stats.drafted grows, per step that emits something, by the rows j in 1 .. T-1 that are not dead; no pads, no forced count.
 * Behind the drafts the step is zgml_hip_resident_decode_speculative_constrained's, all of it: the constrained picks under
 *   row_state[j], acceptance, the dead-end cut, stop tokens, penalties over the call's device history, `logprobs`,
 *   `top_logprobs`, the result getters, the advance of the state word over exactly the emitted tokens. top_k = 1 is the greedy
 *   form. Idle steps make every row dead; their draft executions repeat one token.
 * Exactness. Every emitted token is the target's constrained pick over a confirmed context at its own position and state. The
 *   drafts — masked or not — change how many steps run, never which tokens come out.
 * With no constraint attached to the target the call IS zgml_hip_resident_decode_speculative_model with `sampling`: same tokens,
 *   statistics, launches and graphs.
 * Launches. One graph launch per step: [draft launch] T x { [draft prep] [draft plan] [masked argmax stage 1] [stage 2 +
 *   constrained draft advance] } [prep, T columns] [target plan] [constrained-rows select] [merge + pick] ([log-probability
 *   launches]) [accept] — no launch more than zgml_hip_resident_decode_speculative_model with `sampling`. The graphs belong to the
 *   (target, draft) pair, one per form; the automaton's pointers and the state live in the target's device table, so attaching
 *   another automaton, or none, between calls re-captures nothing, and other calls on either program alternate with this one.
 *   Runtime profile: the target counts plan + 3 + tail launches per step, the draft T x (plan + 3).
 * Blocking. Returns 0. Refused with -1 and an error on the context, before anything is enqueued: sampling == NULL; everything
 *   zgml_hip_resident_decode_speculative_model with `sampling` refuses except the target's constraint — a constraint attached to
 *   the DRAFT stays refused. The state on entry is what zgml_hip_program_set_constraint accepted or an earlier call left.
 *   n_tokens = 0 returns 0 and touches nothing. */
int zgml_hip_resident_decode_speculative_model_constrained(zgml_hip_ctx* ctx, zgml_hip_program* target, zgml_hip_program* draft,
                                                           uint32_t first_token, uint32_t start_pos, uint32_t n_tokens,
                                                           const uint32_t* history /* [n_history] */, uint32_t n_history /* 0 or start_pos */,
                                                           const zgml_sampling* sampling /* not NULL */, int64_t* tokens_out /* [n_tokens] */,
                                                           uint32_t* n_produced /* may be NULL */, zgml_spec_stats* stats /* may be NULL */);

/* ── A draft model under batching: B sequences, one graph. The call above for every sequence of a batched plan, and a sibling of
 * zgml_hip_resident_decode_batch_speculative and _batch_speculative_sampled, not a mode of them: those keep refusing mode > 1.
 * Programs. `target` is a batched plan of n_seqs = B sequences with tokens_per_seq = T >= 2 and a resident set-up, as for
 *   zgml_hip_resident_decode_batch_speculative; `draft` a batched plan of the same context with the same n_seqs, tokens_per_seq =
 *   1, a resident set-up of its own and the target's vocabulary — every other dimension, the weight kind and the KV form (f32
 *   slabs or int8 caches) may differ.
 * Rule. Per sequence that of zgml_hip_resident_decode_speculative_model: at (hist_b[pos_b], pos_b), c[0] = hist_b[pos_b];
 *   execution j of the draft runs sequence b on c[j] at pos_b + j and stores its KV column; c[j + 1] = d[j], the first maximum
 *   of the draft's logits row b, for j < T - 1; the T-th execution exists for its column alone. Acceptance, emission, the stop
 *   cut, the statistics (drafted += T - 1 per emitting step, no pads) and resuming are those of the batched siblings. The other
 *   sequences change neither a sequence's tokens nor its statistics.
 * Idling. A sequence that has its count (n_tokens[b] = 0 is allowed) idles at its END position, as in the batched siblings: it
 *   hands the draft (hist[pos], pos) and the draft idles from there; both programs' T columns from there on are unspecified.
 *   Hence, for every b and BOTH programs: start_pos[b] + n_tokens[b] + T <= max_seq.
 * sampling = NULL: the greedy verify step. Else one zgml_sampling per sequence and the step of
 *   zgml_hip_resident_decode_batch_speculative_sampled, all of it: per-sequence parameters, seeds and stop tokens, penalties over
 *   the device history, `logprobs` (zgml_hip_logprobs_result: [n_seqs][max_tokens]); `top_logprobs` is ignored, as there. The
 *   drafts stay the draft's GREEDY tokens. top_k = 1 with neutral penalties gives the tokens and statistics of the greedy form.
 * Launches. One graph launch per step, a linear chain: [draft launch, B workgroups] T x { [draft batch prep] [draft plan]
 *   [argmax stage 1, grid (nblk, B)] [stage 2 + draft advance, grid (1, B)] } [prep, B T columns] [target plan] [argmax stage 1
 *   over B T rows | the sampled tail] [accept, B workgroups] — T draft executions per step whatever B. The graphs belong to the
 *   (target, draft) pair, one per form, in slots no other call can use on a batched plan: other calls on either program
 *   alternate with this one and invalidate nothing; another draft — or the same one freed, set up again or rebuilt — re-captures.
 *   Runtime profile: the target counts plan + 3 + tail launches per step, the draft T x (plan + 3).
 * Blocking. Returns 0. Refused with -1 and an error on the context that names the sequence where there is one, before anything
 *   is enqueued: everything zgml_hip_resident_decode_batch_speculative (with `sampling`: _sampled) refuses of the target and the
 *   requests (histories[b] / n_history[b] as its per_seq[b].history / n_history); a sharded target; a draft that is NULL, the
 *   target itself, of another context, without a resident set-up, plain, tokens_per_seq != 1, of another n_seqs, sharded or of
 *   another vocabulary; the bound above on either program; a constraint attached to any sequence of either program. All
 *   n_tokens zero returns 0 and touches nothing. */
int zgml_hip_resident_decode_batch_speculative_model(zgml_hip_ctx* ctx, zgml_hip_program* target, zgml_hip_program* draft,
                                                     const uint32_t* first_tokens, const uint32_t* start_pos, const uint32_t* n_tokens,
                                                     uint32_t max_tokens, const uint32_t* const* histories /* [n_seqs] or NULL; entry NULL: none */,
                                                     const uint32_t* n_history /* [n_seqs]: 0 or start_pos[b] */,
                                                     const zgml_sampling* sampling /* [n_seqs], or NULL: greedy verify */,
                                                     int64_t* tokens_out /* [n_seqs][max_tokens] */, uint32_t* n_produced /* [n_seqs] or NULL */,
                                                     zgml_spec_stats* stats /* [n_seqs] or NULL */);

/* Mat-vec roofline micro-benchmark: builds `n_matrices` distinct K x N quantized
 * matrices on the device from the deterministic synthetic generator (q4: nibbles in [-8,7];
 * otherwise int8), runs `warmup` + `iters` launches round-robin over the ring and returns the
 * average kernel time in microseconds measured with HIP events on the launch stream (<0 on
 * error). `bytes_per_launch` receives the algorithmic bytes (K*N/32*{18|34} + 4K + 4N). */
double zgml_hip_qmatvec_bench(zgml_hip_ctx* ctx, uint32_t K, uint32_t N, int q4, uint32_t n_matrices,
                              uint32_t warmup, uint32_t iters, uint64_t* bytes_per_launch);
/* A CHAIN of square (K x K) mat-vecs with a true data dependency: launch i computes y_i = (x_i^T W_i) * c (an
 * epilogue multiply by a constant vector keeps magnitudes bounded) and launch i + 1 reads y_i as its x (ping-pong
 * vectors; n_matrices even). The roofline figure of bench.py: launches are ordered by DATA, not only by the stream.
 * Microseconds per launch (< 0 on error). */
double zgml_hip_qmatvec_chain_bench(zgml_hip_ctx* ctx, uint32_t K, int q4, uint32_t n_matrices, uint32_t warmup, uint32_t iters,
                                    uint64_t* bytes_per_launch);
/* Same ring with M input rows (M > 1 runs the f32-MFMA tile kernel used by prefill plans);
 * bytes = weights + 4*M*K + 4*M*N, flops = 2*M*K*N. */
double zgml_hip_qmatmul_bench(zgml_hip_ctx* ctx, uint32_t M, uint32_t K, uint32_t N, int q4, uint32_t n_matrices,
                              uint32_t warmup, uint32_t iters, uint64_t* bytes_per_launch);
/* The same ring of M = 1 mat-vecs as independent launches: the captured graph forks the ring over n_streams
 * branches (distinct outputs), so launches may overlap on the device. Not the decode path (every mat-vec there
 * waits for its predecessor); it separates what the kernel can stream from what a dependent launch of this size
 * costs. Returns microseconds per launch (< 0 on error). */
double zgml_hip_qmatvec_overlap_bench(zgml_hip_ctx* ctx, uint32_t K, uint32_t N, int q4, uint32_t n_matrices, uint32_t n_streams,
                                      uint32_t iters, uint64_t* bytes_per_launch);
/* ... and on EXPLICIT streams: stream t replays its own graph of the matrices i = t (mod n_streams), all n_streams replays
 * in flight at once on their own queues (n_matrices % n_streams == 0). Microseconds per launch over all streams. */
double zgml_hip_qmatvec_streams_bench(zgml_hip_ctx* ctx, uint32_t K, uint32_t N, int q4, uint32_t n_matrices, uint32_t n_streams,
                                      uint32_t iters, uint64_t* bytes_per_launch);
/* Ring benchmark of the f16-promoted dense matmul (M == 1: f32 x times f16 weights; M > 1: f16
 * MFMA); bytes = 2*K*N + 4*M*K + 4*M*N. N % 16 == 0. */
double zgml_hip_dense_f16_bench(zgml_hip_ctx* ctx, uint32_t M, uint32_t K, uint32_t N, uint32_t n_matrices,
                                uint32_t warmup, uint32_t iters, uint64_t* bytes_per_launch);
/* One mat-vec y = x^T W with synthetic matrix `matrix_id` of the same generator (parity tests
 * rebuild that matrix on the host in int8 + f32-scale form and check y against the oracle).
 * Returns 0 on success. */
int zgml_hip_qmatvec_synth(zgml_hip_ctx* ctx, uint32_t K, uint32_t N, int q4, uint32_t matrix_id,
                           const float* x_host, float* y_host);
/* Device-to-device float4 copy of `bytes` bytes, average microseconds per launch (the measured
 * "achievable HBM" yardstick printed next to the 8 TB/s nominal peak). */
double zgml_hip_copy_bench(zgml_hip_ctx* ctx, uint64_t bytes, uint32_t warmup, uint32_t iters);

#ifdef __cplusplus
}
#endif
#endif /* ZGML_HIP_H */
