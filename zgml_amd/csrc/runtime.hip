// runtime.hip — the C ABI of include/zgml_hip.h: context, program compile / refresh / execute,
// host dense-matmul override, profiling counters and the measurement extensions.
//
// Execution model (MI355X-first, not a translation of the Metal/WGPU backends):
//   * one HIP stream per context; a compiled program is a fixed launch list captured once into a
//     hipGraph and replayed per token (decode is launch-bound: ~1.7k DeviceOps per SmolLM token);
//   * the two per-step dynamic fields of the reference (slice_assign.dst_offset and
//     attention.seq_kv, src/device_inference.zig:242-256) live in a device-resident word per op
//     ("dyn block") that kernels dereference, so refresh_program never re-records the graph;
//   * per-step inputs are packed into one pinned staging buffer, moved with ONE H2D copy and
//     scattered on the device; outputs are gathered the same way (the reference's per-token
//     traffic is 32 small uploads + one logits download, src/llama_inference.zig:405-466);
//   * quantized weights are re-packed on the device at compile time (qmatvec.hip) and buffers no
//     op references (the dead f32 master copies of quantized weights) are neither
//     allocated nor uploaded.
// There is no CPU fallback anywhere: every DeviceOp kind has a kernel.
#include "runtime_internal.h"

namespace zgml_rt {
std::string g_create_error;
}

namespace {


// ── Capabilities.hip ────────────────────────────────────────────────────────────────────────
void fill_caps(zgml_capabilities* c) {
    memset(c, 0, sizeof(*c));
    c->compiled_programs = 1;
    c->host_visible_program_memory = 0; // discrete HBM: no per-op CPU fallback is possible
    c->dense_matmul_f32 = 1;
    c->dense_matmul_f16 = 1;
    c->qmatmul = 1;
    c->fused_elementwise = 1;
    c->max_fused_elementwise_steps_has = 1;
    c->max_fused_elementwise_steps = kMaxFusedSteps;
    c->f16_weight_promotion = 1; // opt-in via ZGML_HIP_OPT_F16_DENSE_WEIGHTS
    c->dynamic_program_refresh = 1;
    c->prefill_attention = 1;
    c->decode_attention = 1;
    c->quantized_kv = 1; // extension ops kvq_store / attention_kvq (include/zgml_hip.h)
    c->command_buffer_execution = 1;
    c->attention_supported = 1;
    c->attention_max_seq_kv_has = 0; // online softmax over key tiles: no score-buffer cap
    c->attention_max_d_head_has = 1;
    c->attention_max_d_head = 512;
}

// packed-GGUF pass-through (include/zgml_hip.h): 0 = reference form, 1 = Q4_0 blocks, 2 = Q8_0 blocks
int gguf_form(const zgml_qweight_upload& qw) {
    if (qw.scales || qw.scales_len || qw.block_size != 32 || !qw.data) return 0;
    const uint64_t n = qw.rows * qw.cols;
    if (!n || n % 32 || qw.cols % 32 || !qweight_packable(qw.rows, qw.cols, 32)) return 0;
    if (qw.data_len == n / 32 * ZGML_QW_GGUF_Q4_0_BLOCK_BYTES) return 1;
    if (qw.data_len == n / 32 * ZGML_QW_GGUF_Q8_0_BLOCK_BYTES) return 2;
    return 0;
}

bool elementwise_op_ok(uint32_t op) { return op >= ZGML_OP_ADD && op <= ZGML_OP_GELU; }

// buffer ids an op touches (opBuffersValid, src/backend.zig:303-325)
void op_buffers(const zgml_device_op& op, std::vector<uint16_t>& out) {
    switch (op.kind) {
        case ZGML_DOP_ELEMENTWISE:
            out.insert(out.end(), {op.u.elementwise.dst, op.u.elementwise.src0, op.u.elementwise.src1});
            break;
        case ZGML_DOP_MATMUL: out.insert(out.end(), {op.u.matmul.dst, op.u.matmul.a, op.u.matmul.b}); break;
        case ZGML_DOP_QMATMUL: out.insert(out.end(), {op.u.qmatmul.dst, op.u.qmatmul.input}); break;
        case ZGML_DOP_SOFTMAX:
        case ZGML_DOP_LAYERNORM:
        case ZGML_DOP_RMSNORM: out.insert(out.end(), {op.u.softmax.dst, op.u.softmax.src}); break;
        case ZGML_DOP_REDUCE: out.insert(out.end(), {op.u.reduce.dst, op.u.reduce.src}); break;
        case ZGML_DOP_REPEAT: out.insert(out.end(), {op.u.repeat.dst, op.u.repeat.src}); break;
        case ZGML_DOP_SLICE_ASSIGN: out.insert(out.end(), {op.u.slice_assign.dst, op.u.slice_assign.src}); break;
        case ZGML_DOP_ROPE: out.insert(out.end(), {op.u.rope.dst, op.u.rope.src, op.u.rope.cos_sin}); break;
        case ZGML_DOP_ATTENTION:
            out.insert(out.end(), {op.u.attention.dst, op.u.attention.q, op.u.attention.k, op.u.attention.v,
                                   op.u.attention.mask});
            break;
        case ZGML_DOP_FUSED_ELEMENTWISE: {
            const auto& fe = op.u.fused_elementwise;
            out.insert(out.end(), {fe.dst, fe.src});
            for (uint32_t s = 0; s < fe.n_steps; s++)
                if (fe.steps[s].op == ZGML_OP_ADD || fe.steps[s].op == ZGML_OP_MUL) out.push_back(fe.steps[s].secondary_buf);
            break;
        }
        case ZGML_DOP_KVQ_STORE: out.insert(out.end(), {op.u.kvq_store.cache, op.u.kvq_store.src}); break;
        case ZGML_DOP_ATTENTION_KVQ:
            out.insert(out.end(), {op.u.attention_kvq.dst, op.u.attention_kvq.q, op.u.attention_kvq.k, op.u.attention_kvq.v,
                                   op.u.attention_kvq.mask});
            break;
        default: break;
    }
}

// DeviceProgram.isSupportedBy(Capabilities.hip), src/backend.zig:277-297
bool program_supported(const zgml_device_program* pr) {
    if (!pr) return false;
    if ((uint64_t)pr->n_buffers != pr->n_buffer_sizes) return false;
    std::vector<uint16_t> ids;
    for (uint64_t i = 0; i < pr->n_ops; i++) {
        const zgml_device_op& op = pr->ops[i];
        if (op.kind == ZGML_DOP_FUSED_ELEMENTWISE && op.u.fused_elementwise.n_steps && !op.u.fused_elementwise.steps) return false;
        if (op.kind == ZGML_DOP_FUSED_ELEMENTWISE && op.u.fused_elementwise.n_steps > (uint32_t)kMaxFusedSteps) return false;
        ids.clear(); // buffer ids first: the per-kind checks below index buffer_sizes with them
        op_buffers(op, ids);
        for (uint16_t id : ids)
            if ((uint64_t)id >= pr->n_buffer_sizes) return false;
        switch (op.kind) {
            case ZGML_DOP_ELEMENTWISE:
                if (!elementwise_op_ok(op.u.elementwise.op)) return false;
                break;
            case ZGML_DOP_MATMUL:
            case ZGML_DOP_SOFTMAX:
            case ZGML_DOP_LAYERNORM:
            case ZGML_DOP_RMSNORM:
            case ZGML_DOP_REPEAT:
            case ZGML_DOP_SLICE_ASSIGN:
            case ZGML_DOP_ROPE: break;
            case ZGML_DOP_QMATMUL: {
                const auto& q = op.u.qmatmul;
                if ((uint64_t)q.weight_idx >= pr->n_qweights) return false;
                const zgml_qweight_upload& qw = pr->qweights[q.weight_idx];
                if (qw.block_size == 0) return false;
                if (qw.rows != q.K || qw.cols != q.N) return false;
                const uint64_t n_elems = (uint64_t)q.K * q.N;
                const uint64_t n_blocks = (n_elems + qw.block_size - 1) / qw.block_size;
                if (gguf_form(qw)) break; // packed-GGUF pass-through, validated by gguf_form()
                if (qw.data_len < n_elems || qw.scales_len < n_blocks) return false;
                break;
            }
            case ZGML_DOP_REDUCE:
                if (op.u.reduce.op != ZGML_OP_SUM && op.u.reduce.op != ZGML_OP_MAX) return false;
                break;
            case ZGML_DOP_ATTENTION:
                if (op.u.attention.d_head > 512) return false;
                break;
            case ZGML_DOP_KVQ_STORE: { // extension ops: quantised KV cache
                const auto& st = op.u.kvq_store;
                if (!st.block_size || st.block_size % 4 || st.d_head % st.block_size || ((uint64_t)st.n_cols * st.d_head) % 4) return false;
                if ((uint64_t)st.n_cols * st.d_head / 4 + (uint64_t)st.n_cols * (st.d_head / st.block_size) > pr->buffer_sizes[st.cache]) return false;
                break;
            }
            case ZGML_DOP_ATTENTION_KVQ: {
                const auto& a = op.u.attention_kvq;
                if (!a.block_size || a.block_size % 4 || a.d_head % a.block_size || ((uint64_t)a.n_cols * a.d_head) % 4) return false;
                if (a.d_head < 16 || a.d_head > 256 || (a.d_head & (a.d_head - 1))) return false; // kernel instances: 16..256, power of two
                if (a.q_off % 4 || a.q_cs % 4 || a.dst_off % 4 || a.dst_cs % 4) return false;    // float4 access to q / dst
                const uint64_t need = (uint64_t)a.n_cols * a.d_head / 4 + (uint64_t)a.n_cols * (a.d_head / a.block_size);
                if (need > pr->buffer_sizes[a.k] || need > pr->buffer_sizes[a.v]) return false;
                break;
            }
            case ZGML_DOP_FUSED_ELEMENTWISE: {
                const auto& fe = op.u.fused_elementwise;
                if (fe.n_steps > (uint32_t)kMaxFusedSteps) return false;
                for (uint32_t s = 0; s < fe.n_steps; s++)
                    if (!elementwise_op_ok(fe.steps[s].op)) return false;
                break;
            }
            default: return false;
        }
    }
    return true;
}

// ── small device helpers ────────────────────────────────────────────────────────────────────
// (blockIdx.y strides over a row: a prefill chunk's token rows are one transfer of 512 KB — one workgroup walking that alone took
// 200 us from device memory and 680 us from mapped host memory)
__global__ void scatter_words_kernel(const IoTableDev* table, const uint32_t* stage) {
    const IoTableDev e = table[blockIdx.x];
    uint32_t* dst = (uint32_t*)e.dev;
    const uint32_t* src = stage + e.stage_off_words;
    for (uint32_t i = blockIdx.y * blockDim.x + threadIdx.x; i < e.n_words; i += blockDim.x * gridDim.y) dst[i] = src[i];
}
// (blockIdx.y strides over a row: the logits of a decode step are one row of ~50k words)
__global__ void gather_words_wide_kernel(const IoTableDev* table, uint32_t* stage) {
    const IoTableDev e = table[blockIdx.x];
    const uint32_t* src = (const uint32_t*)e.dev;
    uint32_t* dst = stage + e.stage_off_words;
    for (uint32_t i = blockIdx.y * blockDim.x + threadIdx.x; i < e.n_words; i += blockDim.x * gridDim.y) dst[i] = src[i];
}

uint32_t io_grid_y(uint32_t max_row_words) { return std::max<uint32_t>(1, std::min<uint32_t>(64, max_row_words / 1024)); } // workgroups per transfer row

} // namespace

namespace zgml_rt {
// Diagnostics: ZGML_HIP_GRAPH_DUMP=<dir> writes <dir>/<tag>.dot (hipGraphDebugDotPrint) and prints the node-type
// histogram of every graph the runtime instantiates (how the rocprofv3 crash inside hipGraphLaunch of the per-token
// graph was narrowed down: DESIGN.md section 5).
void dump_graph(hipGraph_t g, const char* tag) {
    const char* dir = sw().hip_graph_dump;
    if (!dir || !g) return;
    size_t n = 0;
    if (hipGraphGetNodes(g, nullptr, &n) != hipSuccess) return;
    std::vector<hipGraphNode_t> nodes(n);
    if (n && hipGraphGetNodes(g, nodes.data(), &n) != hipSuccess) return;
    std::map<int, size_t> hist;
    size_t max_shmem = 0, n_kernel = 0;
    for (hipGraphNode_t nd : nodes) {
        hipGraphNodeType t;
        if (hipGraphNodeGetType(nd, &t) != hipSuccess) continue;
        hist[(int)t]++;
        if (t == hipGraphNodeTypeKernel) {
            hipKernelNodeParams kp{};
            if (hipGraphKernelNodeGetParams(nd, &kp) == hipSuccess) max_shmem = std::max<size_t>(max_shmem, kp.sharedMemBytes), n_kernel++;
        }
    }
    fprintf(stderr, "[zgml_hip] graph %s: %zu nodes;", tag, n);
    for (auto& kv : hist) fprintf(stderr, " type%d=%zu", kv.first, kv.second);
    fprintf(stderr, " (kernel=%d memcpy=%d memset=%d host=%d empty=%d event_record=%d wait_event=%d); max dynamic LDS %zu B over %zu kernel nodes\n",
            (int)hipGraphNodeTypeKernel, (int)hipGraphNodeTypeMemcpy, (int)hipGraphNodeTypeMemset, (int)hipGraphNodeTypeHost,
            (int)hipGraphNodeTypeEmpty, (int)hipGraphNodeTypeEventRecord, (int)hipGraphNodeTypeWaitEvent, max_shmem, n_kernel);
    const std::string path = std::string(dir) + "/" + tag + ".dot";
    hipGraphDebugDotPrint(g, path.c_str(), 0);
}

// Drop every captured graph of the program: both bake the plan's kernel nodes and the device parameter arrays
// build_plan() is about to free, so a plan rebuild must never leave one behind (the resident graph included).
void free_graph(zgml_hip_program* p) {
    for (GraphSlot* g : {&p->io_graph, &p->graph, &p->graph_tail, &p->shard_graph}) g->reset();
    free_resident_graph(p);
}
} // namespace zgml_rt

namespace {

bool ensure_stage(zgml_hip_program* p, uint64_t bytes) {
    if (bytes <= p->stage_cap) return true;
    zgml_hip_ctx* ctx = p->ctx;
    hipStreamSynchronize(ctx->stream);
    p->io_graph.reset(); // (its kernels hold the buffers' addresses)
    if (p->stage_host) hipHostFree(p->stage_host);
    if (p->stage_out_host) hipHostFree(p->stage_out_host);
    if (p->stage_dev) hipFree(p->stage_dev);
    p->stage_host = p->stage_out_host = p->stage_dev = nullptr;
    p->stage_cap = 0; // (a failed regrow below leaves no capacity standing over no buffers)
    uint64_t cap = 1 << 16;
    while (cap < bytes) cap <<= 1;
    if (!CTX_CHECK(ctx, hipHostMalloc(&p->stage_host, cap, hipHostMallocMapped))) return false;
    if (!CTX_CHECK(ctx, hipHostMalloc(&p->stage_out_host, cap, hipHostMallocMapped))) return false;
    if (!CTX_CHECK(ctx, hipMalloc(&p->stage_dev, cap))) return false;
    p->stage_cap = cap;
    return true;
}

// (re)build the cached transfer table when the descriptor list changed
bool prepare_io(zgml_hip_program* p, IoPlan& plan, const zgml_program_io* ios, uint64_t n) {
    if (&plan == &p->in_plan && p->hoist_ok)
        for (uint64_t i = 0; i < n; i++)
            if (ios[i].buf_idx < p->hoist_guard.size() && p->hoist_guard[ios[i].buf_idx]) { // the host writes what a hoisted repeat read or wrote
                p->hoist_ok = false;
                p->plan_dirty = true;
                break;
            }
    bool same = plan.entries.size() == n;
    for (uint64_t i = 0; same && i < n; i++)
        same = plan.entries[i] == IoEntry{ios[i].buf_idx, ios[i].offset, ios[i].size};
    if (same) return true;
    zgml_hip_ctx* ctx = p->ctx;
    hipStreamSynchronize(ctx->stream);
    p->io_graph.reset(); // (captured for the tables that are about to change)
    plan.entries.clear();
    plan.word_aligned = true;
    plan.total_words = 0, plan.max_row_words = 0;
    if (plan.table_dev) hipFree(plan.table_dev);
    plan.table_dev = nullptr;
    std::vector<IoTableDev> table;
    for (uint64_t i = 0; i < n; i++) {
        const zgml_program_io& io = ios[i];
        if (io.buf_idx >= p->bufs.size()) {
            ctx->fail("program I/O names buffer " + std::to_string(io.buf_idx) + " which does not exist");
            return false;
        }
        if (!p->bufs[io.buf_idx]) {
            ctx->fail("program I/O names buffer " + std::to_string(io.buf_idx) +
                      " which has no f32 image on the device: no op references it and it was elided at compile"
                      " time (ZGML_HIP_OPT_SKIP_DEAD_UPLOADS=0 keeps it), or it is a matmul weight promoted to f16");
            return false;
        }
        if ((uint64_t)io.offset + io.size > p->sizes[io.buf_idx] * sizeof(float)) {
            ctx->fail("program I/O out of range for buffer " + std::to_string(io.buf_idx));
            return false;
        }
        plan.entries.push_back({io.buf_idx, io.offset, io.size});
        if ((io.offset & 3) || (io.size & 3)) plan.word_aligned = false;
        table.push_back({(float*)((char*)p->bufs[io.buf_idx] + io.offset), plan.total_words, io.size / 4});
        plan.max_row_words = std::max<uint32_t>(plan.max_row_words, io.size / 4);
        plan.total_words += (io.size + 3) / 4;
    }
    // the input table carries one more row: the program's dynamic words (one per op), so that a refresh's changes ride in the same
    // staging copy and scatter launch as the inputs instead of a transfer of their own (upload_inputs)
    const bool with_dyn = &plan == &p->in_plan && plan.word_aligned && !table.empty() && p->dyn_dev && !p->ops.empty();
    if (with_dyn) table.push_back({(float*)p->dyn_dev, plan.total_words, (uint32_t)p->ops.size()}), plan.max_row_words = std::max<uint32_t>(plan.max_row_words, (uint32_t)p->ops.size());
    if (plan.word_aligned && !table.empty()) {
        if (!CTX_CHECK(ctx, hipMalloc((void**)&plan.table_dev, table.size() * sizeof(IoTableDev)))) return false;
        if (!CTX_CHECK(ctx, h2d_sync(ctx->stream, plan.table_dev, table.data(), table.size() * sizeof(IoTableDev)))) return false;
    }
    plan.dyn_row = with_dyn;
    return ensure_stage(p, ((uint64_t)plan.total_words + (with_dyn ? p->ops.size() : 0)) * 4);
}


void note_seq_kv_bounds(zgml_hip_program* p) {
    p->seq_kv_bound.resize(p->ops.size(), 0);
    for (size_t i = 0; i < p->ops.size(); i++)
        if (const DynField f = dyn_field(p->ops[i]); f.role == DynField::SeqKv) p->seq_kv_bound[i] = std::max(p->seq_kv_bound[i], *f.word);
}

// copy ops (and their fused steps) into program-owned storage
void own_ops(zgml_hip_program* p, const zgml_device_op* ops, uint64_t n_ops) {
    // a static refresh may change an op's kind: bounds of ops that are no longer the same attention start over
    if (p->seq_kv_bound.size() == n_ops && p->ops.size() == n_ops)
        for (uint64_t i = 0; i < n_ops; i++)
            if (p->ops[i].kind != ops[i].kind) p->seq_kv_bound[i] = 0;
    p->ops.assign(ops, ops + n_ops);
    p->dyn_ops.clear(); // the ops whose dynamic field moves (what a per-token refresh touches: zgml_hip_refresh_dynamic)
    for (uint64_t i = 0; i < n_ops; i++)
        if (dyn_field(ops[i]).moves()) p->dyn_ops.push_back((uint32_t)i);
    p->steps.assign(n_ops, {});
    for (uint64_t i = 0; i < n_ops; i++) {
        if (ops[i].kind == ZGML_DOP_FUSED_ELEMENTWISE) {
            const auto& fe = ops[i].u.fused_elementwise;
            p->steps[i].assign(fe.steps, fe.steps + fe.n_steps);
            p->ops[i].u.fused_elementwise.steps = p->steps[i].data();
        }
    }
    note_seq_kv_bounds(p);
}

// bytes of the ACTIVE union member of an op (the rest of the union may be uninitialised padding); 0: unknown kind
size_t payload_bytes(const zgml_device_op& o) {
    switch (o.kind) {
        case ZGML_DOP_ELEMENTWISE: return sizeof(o.u.elementwise);
        case ZGML_DOP_MATMUL: return sizeof(o.u.matmul);
        case ZGML_DOP_QMATMUL: return sizeof(o.u.qmatmul);
        case ZGML_DOP_SOFTMAX:
        case ZGML_DOP_LAYERNORM:
        case ZGML_DOP_RMSNORM: return sizeof(o.u.rmsnorm);
        case ZGML_DOP_REDUCE: return sizeof(o.u.reduce);
        case ZGML_DOP_REPEAT: return sizeof(o.u.repeat);
        case ZGML_DOP_SLICE_ASSIGN: return sizeof(o.u.slice_assign);
        case ZGML_DOP_ROPE: return sizeof(o.u.rope);
        case ZGML_DOP_ATTENTION: return sizeof(o.u.attention);
        case ZGML_DOP_FUSED_ELEMENTWISE: return sizeof(o.u.fused_elementwise);
        case ZGML_DOP_KVQ_STORE: return sizeof(o.u.kvq_store);
        case ZGML_DOP_ATTENTION_KVQ: return sizeof(o.u.attention_kvq);
        default: return 0;
    }
}

// true when the static part of two ops is identical (dynamic fields and step pointers ignored). No copies: the bytes of the
// active union member are compared around the member's dynamic field — this runs once per op per token on the drop-in path
// (refresh_program is called before every execute: src/device_inference.zig:260-263).
bool same_static(const zgml_device_op& a, const zgml_device_op& b) {
    const size_t len = payload_bytes(a);
    if (a.kind != b.kind || !len) return false;
    const char *x = (const char*)&a.u, *y = (const char*)&b.u;
    size_t off = len, flen = 0; // equal but for [off, off + flen)
    // a store with patch_stride == 0 is static: its offset / column is not on p->dyn_ops, so a change must rebuild the plan
    if (const DynField fa = dyn_field(a); fa.moves() && dyn_field(b).moves()) off = (size_t)((const char*)fa.word - x), flen = sizeof(uint32_t);
    if (a.kind == ZGML_DOP_FUSED_ELEMENTWISE) {
        const auto &fa = a.u.fused_elementwise, &fb = b.u.fused_elementwise;
        if (fa.n_steps != fb.n_steps) return false;
        for (uint32_t s = 0; s < fa.n_steps; s++)
            if (fa.steps[s].op != fb.steps[s].op || fa.steps[s].is_swapped != fb.steps[s].is_swapped ||
                fa.steps[s].secondary_buf != fb.steps[s].secondary_buf || fa.steps[s].secondary_offset != fb.steps[s].secondary_offset)
                return false;
        off = offsetof(zgml_op_fused_elementwise, steps), flen = sizeof(fa.steps);
    }
    return memcmp(x, y, off) == 0 && memcmp(x + off + flen, y + off + flen, len - off - flen) == 0;
}

} // namespace

namespace zgml_rt {

// the host mirror of the dynamic block from the ops: the word of every op that has one — the stores with patch_stride 0 included,
// the "static dyn words" the resident loops re-upload from here — and 0 for the rest
void set_dyn_from_ops(zgml_hip_program* p) {
    for (size_t i = 0; i < p->ops.size(); i++) {
        const DynField f = dyn_field(p->ops[i]);
        const uint32_t v = f.word ? *f.word : 0;
        if (p->dyn_host[i] != v) p->dyn_host[i] = v, p->dyn_dirty = true;
    }
}

// rebuild the plan, dropping every graph captured from the old one, when it is dirty or the context's fuse epoch moved
void ensure_plan(zgml_hip_program* p) {
    if (p->plan_dirty || p->fuse_epoch != p->ctx->fuse_epoch) {
        free_graph(p);
        build_plan(p);
    }
}

// `work` captured from stream s (thread-local mode) and instantiated into the empty `slot`; `tag` names the graph for
// ZGML_HIP_GRAPH_DUMP (nullptr: not dumped). false, reported on ctx and with the slot left empty, when any step fails.
bool capture_graph(zgml_hip_ctx* ctx, hipStream_t s, const char* tag, const std::function<void()>& work, GraphSlot* slot) {
    if (!CTX_CHECK(ctx, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal))) return false;
    work();
    if (!CTX_CHECK(ctx, hipStreamEndCapture(s, &slot->graph)) || !slot->graph) return false;
    if (tag) dump_graph(slot->graph, tag);
    hipGraphExec_t ge = nullptr;
    if (!CTX_CHECK(ctx, hipGraphInstantiate(&ge, slot->graph, nullptr, nullptr, 0))) {
        slot->reset();
        return false;
    }
    slot->exec = ge;
    return true;
}

void run_plan(zgml_hip_program* p, hipStream_t s, size_t first, size_t count, DenseHeadTail* tail) {
    // (the rider goes to the plan's last launch alone: nothing behind it rewrites the logits or reads what it prepares ahead)
    const auto run = [&](Launch& L) { tail && L.run_tail && &L == &p->plan.back() ? L.run_tail(s, tail) : L.run(s); };
#ifdef ZGML_TRACE
    // diagnostics build only: ZGML_HIP_SKIP_KINDS=<bitmask of DeviceOp tags> drops those launches (timing ablation
    // only; results are garbage)
    // ZGML_HIP_SKIP_MOD="<period>:<bitmask>" drops launch i >= 1 when bit ((i-1) % period) is set
    static unsigned mod_period = 0, mod_mask = 0;
    static bool mod_init = false;
    if (!mod_init) {
        mod_init = true;
        if (const char* e = sw().hip_skip_mod) sscanf(e, "%u:%x", &mod_period, &mod_mask);
    }
    for (size_t i = first; i < first + count && i < p->plan.size(); i++) {
        if (sw().hip_skip_kinds & (1u << p->plan[i].kind)) continue;
        if (mod_period && i >= 1 && (mod_mask & (1u << ((i - 1) % mod_period)))) continue;
        run(p->plan[i]);
    }
#else
    for (size_t i = first; i < first + count && i < p->plan.size(); i++) run(p->plan[i]);
#endif
}

void flush_dyn(zgml_hip_program* p) {
    if (!p->dyn_dirty || p->ops.empty()) return;
    hipMemcpyAsync(p->dyn_dev, p->dyn_host, p->ops.size() * sizeof(uint32_t), hipMemcpyHostToDevice, p->ctx->stream);
    p->dyn_dirty = false;
}

// enqueue the whole program on the context stream (graph replay when enabled)
void enqueue(zgml_hip_program* p) {
    zgml_hip_ctx* ctx = p->ctx;
    ensure_plan(p);
    flush_dyn(p);
    if (ctx->opt_profile) {
        hipEvent_t e0, e1;
        hipEventCreate(&e0);
        hipEventCreate(&e1);
        for (auto& L : p->plan) {
            hipEventRecord(e0, ctx->stream);
            L.run(ctx->stream);
            hipEventRecord(e1, ctx->stream);
            hipEventSynchronize(e1);
            float ms = 0;
            hipEventElapsedTime(&ms, e0, e1);
            if (L.kind < ZGML_DOP_COUNT) p->profile.time_ns[L.kind] += (uint64_t)(ms * 1e6);
            L.prof_ns += (uint64_t)(ms * 1e6);
            L.prof_calls++;
        }
        hipEventDestroy(e0);
        hipEventDestroy(e1);
        if (sw().hip_debug_plan.value >= 2 && p->plan[0].prof_calls == 8) {
            // per-launch table after 8 profiled executions (first 40 launches: one layer and a bit)
            for (size_t i = 0; i < p->plan.size() && i < 40; i++)
                fprintf(stderr, "[zgml_hip] launch %3zu kind %2u ops %4u [%u..%u]  %.2f us\n", i, p->plan[i].kind, p->plan[i].n_ops,
                        p->plan[i].op_lo, p->plan[i].op_hi, p->plan[i].prof_ns / 1e3 / p->plan[i].prof_calls);
        }
        return;
    }
    if (ctx->opt_graph && !p->plan.empty()) {
        if (!p->graph.exec) {
            // two graphs (zgml_hip_program::graph_tail): the head holds the first sixth of the launches (at least 8: its device
            // time has to cover the host's submission of the tail), short plans stay one graph
            const int split_env = sw().hip_graph_split;
            size_t head = p->plan.size() >= 48 ? std::max<size_t>(8, p->plan.size() / 6) : p->plan.size();
            if (split_env == 0) head = p->plan.size();
            if (split_env > 0) head = std::min<size_t>((size_t)split_env, p->plan.size());
            auto capture = [&](size_t first, size_t count, GraphSlot* slot, const char* tag) {
                return capture_graph(ctx, ctx->stream, tag, [&] { run_plan(p, ctx->stream, first, count); }, slot);
            };
            if (capture(0, head, &p->graph, "program") && head < p->plan.size() && !capture(head, p->plan.size() - head, &p->graph_tail, "program-tail"))
                p->graph.reset(); // (all or nothing: eager below)
        }
        if (p->graph.exec) {
            CTX_CHECK(ctx, hipGraphLaunch(p->graph.exec, ctx->stream));
            if (p->graph_tail.exec) CTX_CHECK(ctx, hipGraphLaunch(p->graph_tail.exec, ctx->stream));
            return;
        }
    }
    run_plan(p, ctx->stream, 0, p->plan.size());
}

// a caller about to touch a buffer some hoisted (run-once) repeat read or wrote: back to running every repeat in the plan
void unhoist_if_guarded(zgml_hip_program* p, uint16_t buf_idx) {
    if (p->hoist_ok && buf_idx < p->hoist_guard.size() && p->hoist_guard[buf_idx]) p->hoist_ok = false, p->plan_dirty = true;
}

} // namespace zgml_rt

namespace {

uint64_t now_ns() {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

bool grow(zgml_hip_ctx* ctx, float** ptr, uint64_t* cap, uint64_t elems) {
    if (elems <= *cap) return true;
    if (*ptr) hipFree(*ptr);
    *ptr = nullptr;
    *cap = 0;
    if (!CTX_CHECK(ctx, hipMalloc((void**)ptr, elems * sizeof(float)))) return false;
    *cap = elems;
    return true;
}

// one op's dynamic field set to `v`: the program's copy, the host mirror of the device word, the attention's compile-time bound;
// false when the value leaves the span the level schedule assumed (dynamic_field_in_bounds)
bool apply_dynamic(zgml_hip_program* p, uint32_t i, uint32_t v) {
    zgml_device_op& op = p->ops[i];
    const DynField f = dyn_field(op);
    if (!f.word) return true;
    *f.word = v;
    if (f.role == DynField::SeqKv && i < p->seq_kv_bound.size()) p->seq_kv_bound[i] = std::max(p->seq_kv_bound[i], v);
    if (p->dyn_host[i] != v) p->dyn_host[i] = v, p->dyn_dirty = true;
    return !p->plan_batched || dynamic_field_in_bounds(p->sched, i, op);
}

// the loop of the two refresh_dynamic entry points: every op on p->dyn_ops takes pos_kv(i) = {slice_pos, seq_kv} of ITS sequence
template <class PosKv>
void refresh_dynamic_ops(zgml_hip_ctx* ctx, zgml_hip_program* p, PosKv pos_kv) {
    const uint64_t t_prof = ctx->host_prof ? now_ns() : 0;
    bool in_bounds = true;
    for (const uint32_t i : p->dyn_ops) {
        const DynField f = dyn_field(p->ops[i]);
        const std::pair<uint32_t, uint32_t> at = pos_kv(i);
        in_bounds = apply_dynamic(p, i, f.role == DynField::SeqKv ? at.second : f.at(at.first, 0)) && in_bounds;
    }
    if (p->plan_batched && !in_bounds) p->batching_safe = false, p->plan_dirty = true;
    if (ctx->host_prof) ctx->prof_ns[0] += now_ns() - t_prof, ctx->prof_calls[0]++;
}

} // namespace

// ════════════════════════════════ C ABI ════════════════════════════════

extern "C" {

zgml_hip_ctx* zgml_hip_create(int device_ordinal) {
    g_create_error.clear();
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) {
        g_create_error = std::string("no HIP device: ") + (e == hipSuccess ? "count is 0" : hipGetErrorString(e));
        return nullptr;
    }
    if (device_ordinal < 0 || device_ordinal >= n) {
        g_create_error = "device ordinal out of range";
        return nullptr;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_ordinal) != hipSuccess) {
        g_create_error = "hipGetDeviceProperties failed";
        return nullptr;
    }
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) {
        g_create_error = std::string("device is ") + prop.gcnArchName + ", this backend is built for gfx950 only";
        return nullptr;
    }
    if (hipSetDevice(device_ordinal) != hipSuccess) {
        g_create_error = "hipSetDevice failed";
        return nullptr;
    }
    zgml_hip_ctx* ctx = new zgml_hip_ctx();
    ctx->device = device_ordinal;
    // environment overrides of the option defaults (profilers: ZGML_HIP_GRAPH=0 traces eager launches)
    read_ctx_switches(*ctx);
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        g_create_error = "hipStreamCreate failed";
        delete ctx;
        return nullptr;
    }
    hipMalloc((void**)&ctx->arg_val, kArgPairs * sizeof(float));
    hipMalloc((void**)&ctx->arg_idx, kArgPairs * sizeof(int64_t));
    hipMalloc((void**)&ctx->arg_out, sizeof(int64_t));
    hipHostMalloc((void**)&ctx->arg_out_host, sizeof(int64_t), hipHostMallocDefault);
    ctx->n_cu = prop.multiProcessorCount;
    // the hand-off flag of the fused launches: pinned + mapped; without it no fusion is built (fuse_qkv_attention)
    if (hipHostMalloc((void**)&ctx->handoff_flag, 64, hipHostMallocMapped) == hipSuccess) {
        memset(ctx->handoff_flag, 0, 64);
        if (hipHostGetDevicePointer((void**)&ctx->handoff_flag_dev, ctx->handoff_flag, 0) != hipSuccess) ctx->handoff_flag_dev = nullptr;
    }
    return ctx;
}

void zgml_hip_shard_destroy(zgml_hip_ctx* ctx);
void zgml_hip_destroy(zgml_hip_ctx* ctx) {
    if (ctx && ctx->host_prof && ctx->prof_calls[1]) {
        static const char* const names[4] = {"refresh", "upload (pack + H2D + scatter)", "enqueue (dynamic words + graph launch)", "download (gather + D2H + wait + unpack)"};
        fprintf(stderr, "[zgml_hip] host time per call of the vtable path's phases:\n");
        for (int k = 0; k < 4; k++)
            if (ctx->prof_calls[k]) fprintf(stderr, "  %-44s %8.2f us x %llu\n", names[k], ctx->prof_ns[k] / 1e3 / ctx->prof_calls[k], (unsigned long long)ctx->prof_calls[k]);
    }
    if (!ctx) return;
    zgml_hip_shard_destroy(ctx);
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    ctx->drop_b_cache();
    free_kv_move_pool(ctx);
    free_kv_park_stage(ctx);
    hipFree(ctx->mm_a);
    hipFree(ctx->mm_b);
    hipFree(ctx->mm_c);
    hipFree(ctx->arg_val);
    hipFree(ctx->arg_idx);
    hipFree(ctx->arg_out);
    hipHostFree(ctx->arg_out_host);
    if (ctx->handoff_flag) hipHostFree(ctx->handoff_flag);
    hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char* zgml_hip_last_error(const zgml_hip_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

void zgml_hip_clear_error(zgml_hip_ctx* ctx) {
    if (ctx) ctx->err.clear();
}

void zgml_hip_capabilities(zgml_capabilities* out) {
    if (out) fill_caps(out);
}

int zgml_hip_program_supported(const zgml_device_program* program) { return program_supported(program) ? 1 : 0; }

int zgml_hip_set_option(zgml_hip_ctx* ctx, int option, int64_t value) {
    if (!ctx) return -1;
    switch (option) {
        case ZGML_HIP_OPT_FUSION: ctx->opt_fusion = value != 0; return 0;
        case ZGML_HIP_OPT_GRAPH: ctx->opt_graph = value != 0; return 0;
        case ZGML_HIP_OPT_PROFILE: ctx->opt_profile = value != 0; return 0;
        case ZGML_HIP_OPT_SKIP_DEAD_UPLOADS: ctx->opt_skip_dead = value != 0; return 0;
        case ZGML_HIP_OPT_F16_DENSE_WEIGHTS: ctx->opt_f16_dense = value != 0; return 0;
        case ZGML_HIP_OPT_ATTN_SPLIT_MIN_KEYS: ctx->opt_attn_split_min_keys = value < 0 ? -1 : value; return 0;
        case ZGML_HIP_OPT_FUSE_RESIDENT_WGS:
            ctx->opt_fuse_resident_wgs = value < 0 ? -1 : value;
            ctx->fuse_epoch++; // existing programs rebuild their plans under the new capacity
            return 0;
        case ZGML_HIP_OPT_KSPLIT: ctx->opt_ksplit = value != 0; return 0; // (latched per program at compile_program)
        case ZGML_HIP_OPT_W8A8: ctx->opt_w8a8 = value != 0; return 0;     // (decides the weights' device format at compile_program)
        case ZGML_HIP_OPT_SMALL_M_MATVEC: // (same) 1: the measured bound; 2..8: that bound
            ctx->opt_small_m = value <= 0 ? 0 : (value == 1 ? kKonRowsRoutedM : (uint32_t)std::min<int64_t>(value, kKonRowsMaxM));
            return 0;
        case ZGML_HIP_OPT_KV_MOVE_NT: ctx->opt_kv_move_nt = value != 0; return 0;
        case ZGML_HIP_OPT_DENSE_WEIGHT_CACHE:
            ctx->b_cache_cap = value > 0 ? (uint64_t)value : 0;
            if (!ctx->b_cache_cap) ctx->drop_b_cache();
            return 0;
        default: return -1;
    }
}

int zgml_hip_dense_matmul_f32(zgml_hip_ctx* ctx, float* dst, uint64_t dst_len, const float* a, uint64_t a_len,
                              const float* b, uint64_t b_len, const zgml_matmul_geom* g) {
    if (!ctx || !g || !dst || !a || !b) return 0;
    if (g->M == 0 || g->N == 0) return 1;
    // spans actually touched (the caller's slices may be larger)
    const uint64_t a_span = g->a_offset + (g->M - 1) * g->a_row_stride + (g->K ? (g->K - 1) * g->a_col_stride : 0) + 1;
    const uint64_t b_span = g->b_offset + (g->K ? (g->K - 1) * g->b_row_stride : 0) + (g->N - 1) * g->b_col_stride + 1;
    const uint64_t c_span = g->dst_offset + (g->M - 1) * g->dst_row_stride + g->N;
    if (a_span > a_len || b_span > b_len || c_span > dst_len) return 0; // caller falls back
    if (g->M > UINT32_MAX || g->N > UINT32_MAX || g->K > UINT32_MAX) return 0;
    hipSetDevice(ctx->device);
    if (!grow(ctx, &ctx->mm_a, &ctx->mm_a_cap, a_span) || !grow(ctx, &ctx->mm_b, &ctx->mm_b_cap, b_span) ||
        !grow(ctx, &ctx->mm_c, &ctx->mm_c_cap, c_span))
        return 0;
    hipStream_t s = ctx->stream;
    if (!CTX_CHECK(ctx, hipMemcpyAsync(ctx->mm_a, a, a_span * 4, hipMemcpyHostToDevice, s))) return 0;
    const float* b_dev = ctx->mm_b;
    bool b_cached = false;
    if (ctx->b_cache_cap && b_span * 4 <= ctx->b_cache_cap) { // weight cache: B stays on the device across calls
        auto it = ctx->b_cache.find(b);
        if (it != ctx->b_cache.end() && it->second.span >= b_span) {
            b_dev = it->second.dev, b_cached = true;
            ctx->b_cache_hits++;
        } else {
            if (it != ctx->b_cache.end()) { // same pointer, larger span now: replace
                ctx->b_cache_bytes -= it->second.span * 4;
                hipFree(it->second.dev);
                ctx->b_cache.erase(it);
            }
            if (ctx->b_cache_bytes + b_span * 4 > ctx->b_cache_cap) ctx->drop_b_cache(); // simplest policy: start over
            float* d = nullptr;
            if (hipMalloc((void**)&d, b_span * 4) == hipSuccess) {
                if (!CTX_CHECK(ctx, hipMemcpyAsync(d, b, b_span * 4, hipMemcpyHostToDevice, s))) {
                    hipFree(d);
                    return 0;
                }
                ctx->b_cache[b] = {d, b_span};
                ctx->b_cache_bytes += b_span * 4;
                b_dev = d, b_cached = true;
            }
            ctx->b_cache_misses++;
        }
    }
    if (!b_cached && !CTX_CHECK(ctx, hipMemcpyAsync(ctx->mm_b, b, b_span * 4, hipMemcpyHostToDevice, s))) return 0;
    // rows of dst may be strided: keep the untouched gaps as the caller has them
    if (g->dst_row_stride != g->N || g->dst_offset != 0)
        if (!CTX_CHECK(ctx, hipMemcpyAsync(ctx->mm_c, dst, c_span * 4, hipMemcpyHostToDevice, s))) return 0;
    DenseMatmulParams dp{};
    dp.dst = ctx->mm_c + g->dst_offset;
    dp.a = ctx->mm_a + g->a_offset;
    dp.b = b_dev + g->b_offset;
    dp.M = (uint32_t)g->M, dp.N = (uint32_t)g->N, dp.K = (uint32_t)g->K;
    dp.a_rs = (uint32_t)g->a_row_stride, dp.a_cs = (uint32_t)g->a_col_stride;
    dp.b_rs = (uint32_t)g->b_row_stride, dp.b_cs = (uint32_t)g->b_col_stride;
    dp.dst_rs = (uint32_t)g->dst_row_stride;
    launch_dense_matmul(s, dp);
    if (!CTX_CHECK(ctx, hipMemcpyAsync(dst, ctx->mm_c, c_span * 4, hipMemcpyDeviceToHost, s))) return 0;
    if (!CTX_CHECK(ctx, hipStreamSynchronize(s))) return 0;
    return 1;
}

void zgml_hip_dense_cache_invalidate(zgml_hip_ctx* ctx, const float* b) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    if (!b) {
        ctx->drop_b_cache();
        return;
    }
    auto it = ctx->b_cache.find(b);
    if (it == ctx->b_cache.end()) return;
    ctx->b_cache_bytes -= it->second.span * 4;
    hipFree(it->second.dev);
    ctx->b_cache.erase(it);
}

void zgml_hip_dense_cache_stats(zgml_hip_ctx* ctx, uint64_t* hits, uint64_t* misses, uint64_t* bytes) {
    if (!ctx) return;
    if (hits) *hits = ctx->b_cache_hits;
    if (misses) *misses = ctx->b_cache_misses;
    if (bytes) *bytes = ctx->b_cache_bytes;
}

zgml_hip_program* zgml_hip_compile_program(zgml_hip_ctx* ctx, const zgml_device_program* prog) {
    if (!ctx || !prog) return nullptr;
    if (!program_supported(prog)) {
        ctx->fail("compile_program: program not supported by Capabilities.hip");
        return nullptr;
    }
    hipSetDevice(ctx->device);
    zgml_hip_program* p = new zgml_hip_program();
    p->ctx = ctx;
    p->ksplit = ctx->opt_ksplit;
    own_ops(p, prog->ops, prog->n_ops);
    const size_t nb = prog->n_buffers;
    p->sizes.resize(nb);
    for (size_t i = 0; i < nb; i++) p->sizes[i] = prog->buffer_sizes[i] ? prog->buffer_sizes[i] : 1;

    // liveness: buffers some op references (F8: the f32 master copy of a quantized weight is not)
    std::vector<char> live(nb, ctx->opt_skip_dead ? 0 : 1);
    std::vector<uint16_t> ids;
    std::vector<char> qw_live(prog->n_qweights, 0);
    for (const auto& op : p->ops) {
        ids.clear();
        op_buffers(op, ids);
        for (uint16_t id : ids) live[id] = 1;
        if (op.kind == ZGML_DOP_QMATMUL) qw_live[op.u.qmatmul.weight_idx] = 1;
    }

    // f16 weight promotion (opt-in; src/backend/wgpu.zig:1071-1104): the B operand of `matmul` ops
    // that has an initial upload is kept only as an MFMA-packed f16 copy. Stricter than the
    // reference, which trusts the first user's geometry: every reader of the buffer must be a
    // matmul using it as B with the same geometry, and no op may write it.
    p->f16_weights.assign(nb, nullptr);
    struct Promo {
        uint64_t K, N, b_off, b_rs, b_cs;
    };
    std::vector<int> promo_state(nb, 0); // 0 unseen, 1 candidate, -1 rejected
    std::vector<Promo> promo(nb);
    if (ctx->opt_f16_dense) {
        std::vector<char> has_upload(nb, 0);
        for (uint64_t i = 0; i < prog->n_initial_uploads; i++)
            if (prog->initial_uploads[i].buf_idx < nb) has_upload[prog->initial_uploads[i].buf_idx] = 1;
        const Schedule acc = build_schedule(p->ops, p->sizes, {});
        for (size_t oi = 0; oi < p->ops.size(); oi++) {
            const auto& op = p->ops[oi];
            for (const Span& sp : acc.access[oi].writes) promo_state[sp.buf] = -1;
            if (op.kind == ZGML_DOP_MATMUL) {
                const auto& m = op.u.matmul;
                const Promo g{m.geom.K, m.geom.N, m.geom.b_offset, m.geom.b_row_stride, m.geom.b_col_stride};
                if (m.a == m.b || m.dst == m.b || !has_upload[m.b] || m.geom.a_col_stride != 1 || !f16_packable(g.K, g.N)) {
                    promo_state[m.b] = -1;
                } else if (promo_state[m.b] == 0) {
                    promo_state[m.b] = 1, promo[m.b] = g;
                } else if (promo_state[m.b] == 1) {
                    const Promo& q = promo[m.b];
                    if (q.K != g.K || q.N != g.N || q.b_off != g.b_off || q.b_rs != g.b_rs || q.b_cs != g.b_cs) promo_state[m.b] = -1;
                }
                promo_state[m.a] = -1;
            } else {
                for (const Span& sp : acc.access[oi].reads) promo_state[sp.buf] = -1;
            }
        }
        for (size_t i = 0; i < nb; i++)
            if (promo_state[i] == 1) live[i] = 0; // no f32 copy on the device
    }

    // one arena for all live buffers, 256-byte aligned slots, zero-initialised like
    // OwnedBufferTable.init (src/backend/reference.zig:81-97)
    uint64_t total = 0;
    std::vector<uint64_t> offs(nb, 0);
    for (size_t i = 0; i < nb; i++) {
        if (!live[i]) continue;
        offs[i] = total;
        total += (p->sizes[i] * sizeof(float) + 255) / 256 * 256;
    }
    bool ok = true;
    if (total) {
        ok = CTX_CHECK(ctx, hipMalloc(&p->arena, total)) && CTX_CHECK(ctx, hipMemsetAsync(p->arena, 0, total, ctx->stream));
    }
    if (ok) ok = CTX_CHECK(ctx, hipMalloc((void**)&p->zero_word, 256)) && CTX_CHECK(ctx, hipMemsetAsync(p->zero_word, 0, 256, ctx->stream));
    p->bufs.assign(nb, nullptr);
    if (ok)
        for (size_t i = 0; i < nb; i++)
            if (live[i]) p->bufs[i] = (float*)((char*)p->arena + offs[i]);

    // initial uploads (skipped for elided buffers)
    for (uint64_t i = 0; ok && i < prog->n_initial_uploads; i++) {
        const zgml_program_io& io = prog->initial_uploads[i];
        if (io.buf_idx >= nb) {
            ctx->fail("initial upload names a buffer that does not exist");
            ok = false;
            break;
        }
        if (!p->bufs[io.buf_idx]) continue;
        if ((uint64_t)io.offset + io.size > p->sizes[io.buf_idx] * sizeof(float)) {
            ctx->fail("initial upload out of range");
            ok = false;
            break;
        }
        ok = CTX_CHECK(ctx, hipMemcpyAsync((char*)p->bufs[io.buf_idx] + io.offset, io.host_ptr, io.size,
                                           hipMemcpyHostToDevice, ctx->stream));
    }

    // promoted weights: stage the f32 image, pack to f16 on the device, drop the f32 image
    uint64_t f16_total = 0;
    for (size_t b = 0; ok && b < nb; b++) {
        if (promo_state[b] != 1) continue;
        const Promo& g = promo[b];
        float* tmp = nullptr;
        void* packed = nullptr;
        const uint64_t bytes = p->sizes[b] * sizeof(float);
        ok = CTX_CHECK(ctx, hipMalloc((void**)&tmp, bytes)) && CTX_CHECK(ctx, hipMemsetAsync(tmp, 0, bytes, ctx->stream)) &&
             CTX_CHECK(ctx, hipMalloc(&packed, f16_packed_bytes(g.K, g.N)));
        if (ok && (g.b_off + (g.K - 1) * g.b_rs + (g.N - 1) * g.b_cs >= p->sizes[b])) {
            ctx->fail("matmul B geometry exceeds its buffer");
            ok = false;
        }
        for (uint64_t i = 0; ok && i < prog->n_initial_uploads; i++) {
            const zgml_program_io& io = prog->initial_uploads[i];
            if (io.buf_idx != b) continue;
            if ((uint64_t)io.offset + io.size > bytes) {
                ctx->fail("initial upload out of range");
                ok = false;
                break;
            }
            ok = CTX_CHECK(ctx, hipMemcpyAsync((char*)tmp + io.offset, io.host_ptr, io.size, hipMemcpyHostToDevice, ctx->stream));
        }
        if (ok) {
            launch_pack_f16(ctx->stream, tmp + g.b_off, (uint32_t)g.b_rs, (uint32_t)g.b_cs, (uint32_t)g.K, (uint32_t)g.N, packed);
            ok = CTX_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        }
        hipFree(tmp);
        if (ok) {
            p->f16_weights[b] = packed;
            p->owned.push_back(packed);
            f16_total += f16_packed_bytes(g.K, g.N);
        } else {
            hipFree(packed);
        }
    }

    p->f16_stream_nt = f16_total >= (192ull << 20);

    // quantized weights: upload raw, classify, then re-pack on the device into TWO arenas (quants, scales)
    // in weight-index order with nothing between consecutive weights: the weights a grouped mat-vec launch
    // reads (q/k/v, gate/up) are then contiguous and the kernel derives every part's pointers from part 0's
    // (preloaded) ones instead of waiting for an argument-block fetch (qmatvec.hip, QMV_HEAD_PARAMS).
    p->qweights.resize(prog->n_qweights);
    uint32_t* flags = nullptr;
    if (ok && prog->n_qweights) ok = CTX_CHECK(ctx, hipMalloc((void**)&flags, 2 * sizeof(uint32_t)));
    struct PendingPack {
        void* raw_a = nullptr; // int8 values, or the GGUF blocks
        float* raw_s = nullptr;
        bool gguf = false;
    };
    std::vector<PendingPack> pending(prog->n_qweights);
    uint64_t qs_total = 0, sc_total = 0;
    // Q4_0-valued weights with f16 scales that only ever feed M = 1 mat-vecs take the K-on-lanes layout (QW_Q4K, qmatvec.hip);
    // a weight an M > 1 matmul reads keeps the n-on-lanes layout the tile kernels are built for. ZGML_HIP_OPT_SMALL_M_MATVEC moves
    // the bound up (M <= 6 by default, at most 8): those row counts have a K-on-lanes kernel of their own (qmatvec_rows.hip)
    p->kon_max_m = ctx->opt_small_m ? ctx->opt_small_m : 1;
    std::vector<char> qw_m1(prog->n_qweights, sw().hip_qmv_kon ? 1 : 0);
    std::vector<char> qw_m1_all(prog->n_qweights, 1); // every use is a dense M = 1 row (the W8A8 arm's condition, reference.zig:512-516)
    for (const auto& op : p->ops)
        if (op.kind == ZGML_DOP_QMATMUL && op.u.qmatmul.weight_idx < prog->n_qweights) {
            const auto& q = op.u.qmatmul;
            if (q.M < 1 || q.M > p->kon_max_m) qw_m1[q.weight_idx] = 0;
            if (q.M != 1 || (q.input_row_stride != 0 && q.input_row_stride != q.K) || (q.dst_row_stride != 0 && q.dst_row_stride != q.N)) qw_m1_all[q.weight_idx] = 0;
        }
    for (uint64_t i = 0; ok && i < prog->n_qweights; i++) {
        if (!qw_live[i]) continue;
        const zgml_qweight_upload& qw = prog->qweights[i];
        QWeightDev& w = p->qweights[i];
        w.K = (uint32_t)qw.rows, w.N = (uint32_t)qw.cols, w.bs = (uint32_t)qw.block_size;
        const uint64_t n_elems = qw.rows * qw.cols;
        const uint64_t n_blocks = (n_elems + qw.block_size - 1) / qw.block_size;
        if (const int form = gguf_form(qw)) { // file blocks straight to the device, unpacked + re-packed there
            w.format = form == 1 ? QW_Q4 : QW_Q8;
            w.scale_f16 = 1;
            pending[i].gguf = true;
            ok = CTX_CHECK(ctx, hipMalloc(&pending[i].raw_a, qw.data_len)) &&
                 CTX_CHECK(ctx, hipMemcpyAsync(pending[i].raw_a, qw.data, qw.data_len, hipMemcpyHostToDevice, ctx->stream));
        } else {
            ok = CTX_CHECK(ctx, hipMalloc(&pending[i].raw_a, n_elems ? n_elems : 1)) &&
                 CTX_CHECK(ctx, hipMalloc((void**)&pending[i].raw_s, (n_blocks ? n_blocks : 1) * sizeof(float))) &&
                 CTX_CHECK(ctx, hipMemcpyAsync(pending[i].raw_a, qw.data, n_elems, hipMemcpyHostToDevice, ctx->stream)) &&
                 CTX_CHECK(ctx, hipMemcpyAsync(pending[i].raw_s, qw.scales, n_blocks * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
            if (!ok) break;
            if (ctx->opt_w8a8 && qw_m1_all[i] && w8a8_applies(qw.rows, qw.cols, qw.block_size)) { // the reference's W8A8 arm (w8a8.hip)
                w.format = QW_W8A8;
                w.KC = (uint32_t)(qw.rows / 32);
                w8a8_packed_bytes(qw.rows, qw.cols, &w.qs_bytes, &w.sc_bytes);
                qs_total += w.qs_bytes, sc_total += w.sc_bytes;
                continue;
            }
            if (!qweight_packable(qw.rows, qw.cols, qw.block_size)) { // odd shapes keep the raw form
                w.format = QW_RAW;
                w.qs = pending[i].raw_a, w.sc = pending[i].raw_s;
                w.qs_bytes = n_elems, w.sc_bytes = n_blocks * 4;
                p->owned.push_back(w.qs);
                p->owned.push_back(w.sc);
                pending[i] = PendingPack{};
                continue;
            }
            const uint32_t cls = classify_qweight(ctx->stream, (const int8_t*)pending[i].raw_a, n_elems, pending[i].raw_s, n_blocks, flags);
            w.format = (cls & 1) ? QW_Q4 : QW_Q8;
            w.scale_f16 = (cls & 2) ? 1 : 0;
        }
        if (!ok) break;
        // (short K stays n-on-lanes: those launches are one latency chain inside the decode stream, where the longer fold of
        // the K-on-lanes tail and the hand-over of the norm cost more than the cheaper inner loop saves: SmolLM-135M
        // 1770 tok/s either way without the hand-over, 1680 with it)
        if (w.format == QW_Q4 && w.scale_f16 && qw_m1[i] && w.K >= (uint32_t)sw().hip_qmv_kon_min_k) w.format = QW_Q4K;
        w.KC = (uint32_t)((qw.rows + 31) / 32);
        packed_bytes(w.format, w.scale_f16, w.K, w.N, &w.qs_bytes, &w.sc_bytes);
        qs_total += w.qs_bytes, sc_total += w.sc_bytes;
    }
    char *qs_arena = nullptr, *sc_arena = nullptr;
    if (ok && qs_total && sw().hip_weight_arena) {
        ok = CTX_CHECK(ctx, hipMalloc((void**)&qs_arena, qs_total)) && CTX_CHECK(ctx, hipMalloc((void**)&sc_arena, sc_total ? sc_total : 16));
        if (qs_arena) p->owned.push_back(qs_arena);
        if (sc_arena) p->owned.push_back(sc_arena);
    }
    uint64_t qs_off = 0, sc_off = 0;
    for (uint64_t i = 0; i < prog->n_qweights; i++) {
        QWeightDev& w = p->qweights[i];
        if (ok && pending[i].raw_a) {
            if (sw().hip_weight_arena) {
                w.qs = qs_arena + qs_off, w.sc = sc_arena + sc_off;
                qs_off += w.qs_bytes, sc_off += w.sc_bytes;
            } else { // experiment: one allocation per weight
                ok = CTX_CHECK(ctx, hipMalloc(&w.qs, w.qs_bytes)) && CTX_CHECK(ctx, hipMalloc(&w.sc, w.sc_bytes));
                if (!ok) break;
                p->owned.push_back(w.qs);
                p->owned.push_back(w.sc);
            }
            if (pending[i].gguf)
                launch_pack_gguf(ctx->stream, (const uint8_t*)pending[i].raw_a, w);
            else if (w.format == QW_W8A8)
                launch_pack_w8a8(ctx->stream, (const int8_t*)pending[i].raw_a, pending[i].raw_s, w);
            else
                launch_pack_qweight(ctx->stream, (const int8_t*)pending[i].raw_a, pending[i].raw_s, w);
        }
    }
    if (ok && prog->n_qweights) ok = CTX_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (auto& pd : pending) { // raw images are only needed until the pack kernels have run
        if (pd.raw_a) hipFree(pd.raw_a);
        if (pd.raw_s) hipFree(pd.raw_s);
    }
    if (flags) hipFree(flags);
    { // weight sets beyond the 256 MB Infinity Cache are streamed with non-temporal loads (see qmatvec.hip: wload)
        uint64_t total = 0;
        for (const QWeightDev& w : p->qweights) total += w.qs_bytes + w.sc_bytes;
        if (total >= sw().hip_nt_min_bytes)
            for (QWeightDev& w : p->qweights) w.stream_nt = 1;
    }

    // split-K scratch shared by all qmatmul launches (they are serialised on one stream)
    for (const auto& op : p->ops)
        if (op.kind == ZGML_DOP_QMATMUL) {
            uint64_t b = qmatmul_scratch_bytes(p->qweights[op.u.qmatmul.weight_idx], op.u.qmatmul.M);
            if (b > p->scratch_bytes) p->scratch_bytes = b;
        } else if (op.kind == ZGML_DOP_MATMUL && op.u.matmul.b < p->f16_weights.size() && p->f16_weights[op.u.matmul.b]) {
            uint64_t b = dense_f16_scratch_bytes((uint32_t)op.u.matmul.geom.M, (uint32_t)op.u.matmul.geom.K); // pre-rounded A operand
            if (b > p->scratch_bytes) p->scratch_bytes = b;
        }
    // the head in front of the block holds the K-split fan-in counters: zero once, every launch re-arms them (kernels.h)
    if (ok && p->scratch_bytes) {
        char* base = nullptr;
        ok = CTX_CHECK(ctx, hipMalloc((void**)&base, kQmmScratchHead + p->scratch_bytes)) && CTX_CHECK(ctx, hipMemsetAsync(base, 0, kQmmScratchHead, ctx->stream));
        if (base) p->scratch = (float*)(base + kQmmScratchHead);
    }

    const size_t n_dyn = p->ops.empty() ? 1 : p->ops.size();
    if (ok)
        ok = CTX_CHECK(ctx, hipMalloc((void**)&p->dyn_dev, n_dyn * sizeof(uint32_t))) &&
             CTX_CHECK(ctx, hipHostMalloc((void**)&p->dyn_host, n_dyn * sizeof(uint32_t), hipHostMallocDefault));
    if (ok) {
        memset(p->dyn_host, 0xFF, n_dyn * sizeof(uint32_t));
        set_dyn_from_ops(p);
        p->dyn_dirty = true;
        build_plan(p);
        ok = CTX_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (!ok) {
        zgml_hip_free_program(ctx, p);
        return nullptr;
    }
    return p;
}

// The per-token refresh reduced to what it is (src/backend/program.zig:7452-7490 StepDynamicParams, as the reference's wgpu backend
// applies it — src/backend/wgpu.zig:1162-1169): every KV store goes to column `slice_pos` and every attention reads `seq_kv` keys
// (schedule.h: dyn_field). O(#dynamic ops); static fields are NOT looked at — a caller that may have changed them calls
// zgml_hip_refresh_program.
int zgml_hip_refresh_dynamic(zgml_hip_ctx* ctx, zgml_hip_program* p, uint32_t slice_pos, uint32_t seq_kv) {
    if (!ctx || !p) return -1;
    refresh_dynamic_ops(ctx, p, [&](uint32_t) { return std::make_pair(slice_pos, seq_kv); });
    return 0;
}

// Batched decode: which sequence each dynamic op follows. Every op on p->dyn_ops must be covered.
int zgml_hip_program_set_sequences(zgml_hip_ctx* ctx, zgml_hip_program* p, uint32_t n_seqs, const uint32_t* dyn_op_indices, const uint32_t* dyn_op_seq,
                                   uint64_t n_dyn) {
    if (!ctx || !p) return -1;
    if (n_seqs < 1 || n_seqs > 32 || (n_dyn && (!dyn_op_indices || !dyn_op_seq))) {
        ctx->fail("set_sequences: n_seqs must be 1..32 and the op lists present");
        return -1;
    }
    std::vector<uint32_t> op_seq(p->ops.size(), UINT32_MAX);
    for (uint64_t k = 0; k < n_dyn; k++) {
        if (dyn_op_indices[k] >= p->ops.size() || dyn_op_seq[k] >= n_seqs) {
            ctx->fail("set_sequences: entry " + std::to_string(k) + " names op " + std::to_string(dyn_op_indices[k]) + " / sequence " +
                      std::to_string(dyn_op_seq[k]) + " outside the program / the " + std::to_string(n_seqs) + " sequences");
            return -1;
        }
        op_seq[dyn_op_indices[k]] = dyn_op_seq[k];
    }
    for (const uint32_t i : p->dyn_ops)
        if (op_seq[i] == UINT32_MAX) {
            ctx->fail("set_sequences: op " + std::to_string(i) + " has a position-dependent field but no sequence was declared for it");
            return -1;
        }
    hipSetDevice(ctx->device);
    free_resident(p); // (a resident set-up reads the declaration: set it up again afterwards)
    p->n_seqs = n_seqs;
    p->op_seq = std::move(op_seq);
    return 0;
}

// zgml_hip_refresh_dynamic per sequence: the ops of sequence b take slice_pos[b] / seq_kv[b]
int zgml_hip_refresh_dynamic_batch(zgml_hip_ctx* ctx, zgml_hip_program* p, const uint32_t* slice_pos, const uint32_t* seq_kv) {
    if (!ctx || !p || !slice_pos || !seq_kv) return -1;
    if (!p->n_seqs) {
        ctx->fail("refresh_dynamic_batch: no sequences declared for this program (zgml_hip_program_set_sequences)");
        return -1;
    }
    refresh_dynamic_ops(ctx, p, [&](uint32_t i) { return std::make_pair(slice_pos[p->op_seq[i]], seq_kv[p->op_seq[i]]); });
    return 0;
}

void zgml_hip_refresh_program(zgml_hip_ctx* ctx, zgml_hip_program* p, const zgml_device_op* ops, uint64_t n_ops) {
    if (!ctx || !p || !ops) return;
    const uint64_t t_prof = ctx->host_prof ? now_ns() : 0;
    bool static_same = n_ops == p->ops.size();
    for (uint64_t i = 0; static_same && i < n_ops; i++) static_same = same_static(p->ops[i], ops[i]);
    if (static_same) {
        // the common per-token case: only dynamic fields moved — of the ops that have one (p->dyn_ops)
        bool in_bounds = true;
        for (const uint32_t i : p->dyn_ops) in_bounds = apply_dynamic(p, i, *dyn_field(ops[i]).word) && in_bounds;
        if (p->plan_batched && !in_bounds) {
            // a dynamic field left the span the level schedule assumed: the reordered plan is no
            // longer provably equivalent, fall back to program order for good
            p->batching_safe = false;
            p->plan_dirty = true;
        }
        if (ctx->host_prof) ctx->prof_ns[0] += now_ns() - t_prof, ctx->prof_calls[0]++;
        return;
    }
    if (n_ops != p->ops.size()) {
        ctx->fail("refresh_program: op list length changed");
        return;
    }
    // a static field changed: legal for the reference's CPU backend (it re-reads ops every
    // execute, src/backend/cpu.zig:128-131), so honour it by rebuilding the launch list
    for (uint64_t i = 0; i < n_ops; i++) {
        // ... except where compile_program specialised a weight's layout on the op list it was given: a Q4_0 weight that only
        // fed M = 1 mat-vecs was packed K-on-lanes (QW_Q4K), which the M > 1 tile kernels cannot read. Refuse the refresh (the
        // program keeps its previous ops) instead of skipping the launch later: a stale destination must never look like success.
        const zgml_device_op& op = ops[i];
        if (op.kind != ZGML_DOP_QMATMUL || op.u.qmatmul.weight_idx >= p->qweights.size()) continue;
        const QWFormat fmt = p->qweights[op.u.qmatmul.weight_idx].format;
        const uint32_t max_m = fmt == QW_Q4K ? p->kon_max_m : 1; // (W8A8: M = 1 only)
        if ((fmt == QW_Q4K || fmt == QW_W8A8) && op.u.qmatmul.M != 1 && op.u.qmatmul.M > max_m) {
            ctx->fail("refresh_program: op " + std::to_string(i) + " turns weight " + std::to_string(op.u.qmatmul.weight_idx) +
                      " into the operand of an M = " + std::to_string(op.u.qmatmul.M) +
                      " qmatmul, but the weight was packed for M <= " + std::to_string(max_m) + " mat-vecs at compile time (" +
                      (fmt == QW_Q4K ? "K-on-lanes" : "W8A8") + " layout): recompile the program");
            return;
        }
    }
    hipStreamSynchronize(ctx->stream);
    own_ops(p, ops, n_ops);
    set_dyn_from_ops(p);
    p->plan_dirty = true;
    if (p->n_seqs) // a static refresh may have made another op dynamic: the declaration only survives while it still covers them all
        for (const uint32_t i : p->dyn_ops)
            if (i >= p->op_seq.size() || p->op_seq[i] == UINT32_MAX) {
                free_resident(p);
                p->n_seqs = 0, p->op_seq.clear();
                break;
            }
}

// inputs: pack -> one H2D -> scatter kernel
static bool upload_inputs(zgml_hip_ctx* ctx, zgml_hip_program* p, const zgml_program_io* inputs, uint64_t n_inputs) {
    hipStream_t s = ctx->stream;
    if (!prepare_io(p, p->in_plan, inputs, n_inputs)) return false;
    if (!n_inputs) return true;
    if (p->in_plan.word_aligned) {
        char* st = (char*)p->stage_host;
        uint64_t off = 0;
        for (uint64_t i = 0; i < n_inputs; i++) {
            memcpy(st + off, inputs[i].host_ptr, inputs[i].size);
            off += (inputs[i].size + 3) / 4 * 4;
        }
        uint32_t rows = (uint32_t)n_inputs;
        if (p->in_plan.dyn_row && p->dyn_dirty) { // the refreshed dynamic words ride along (prepare_io: the table's last row)
            memcpy(st + off, p->dyn_host, p->ops.size() * sizeof(uint32_t));
            off += p->ops.size() * sizeof(uint32_t);
            rows++;
            p->dyn_dirty = false;
        }
        hipMemcpyAsync(p->stage_dev, p->stage_host, off, hipMemcpyHostToDevice, s);
        scatter_words_kernel<<<dim3(rows, io_grid_y(p->in_plan.max_row_words)), 256, 0, s>>>(p->in_plan.table_dev, (const uint32_t*)p->stage_dev);
    } else {
        for (uint64_t i = 0; i < n_inputs; i++)
            hipMemcpyAsync((char*)p->bufs[inputs[i].buf_idx] + inputs[i].offset, inputs[i].host_ptr, inputs[i].size,
                           hipMemcpyHostToDevice, s);
    }
    return true;
}

// outputs: gather kernel -> one D2H -> sync -> unpack
static bool download_outputs(zgml_hip_ctx* ctx, zgml_hip_program* p, const zgml_program_io* outputs, uint64_t n_outputs) {
    hipStream_t s = ctx->stream;
    if (!prepare_io(p, p->out_plan, outputs, n_outputs)) return false;
    if (n_outputs) {
        if (p->out_plan.word_aligned && n_outputs == 1) { // (the decode step: the logits) straight from the buffer, no gather launch in front
            hipMemcpyAsync(p->stage_host, (char*)p->bufs[outputs[0].buf_idx] + outputs[0].offset, outputs[0].size, hipMemcpyDeviceToHost, s);
        } else if (p->out_plan.word_aligned) {
            gather_words_wide_kernel<<<dim3((uint32_t)n_outputs, io_grid_y(p->out_plan.max_row_words)), 256, 0, s>>>(p->out_plan.table_dev, (uint32_t*)p->stage_dev);
            hipMemcpyAsync(p->stage_host, p->stage_dev, (uint64_t)p->out_plan.total_words * 4, hipMemcpyDeviceToHost, s);
        } else {
            for (uint64_t i = 0; i < n_outputs; i++)
                hipMemcpyAsync(outputs[i].host_ptr, (char*)p->bufs[outputs[i].buf_idx] + outputs[i].offset,
                               outputs[i].size, hipMemcpyDeviceToHost, s);
        }
    }
    const uint64_t t0 = now_ns();
    const bool ok = CTX_CHECK(ctx, hipStreamSynchronize(s)) && ctx->handoff_ok("execute_program");
    p->profile.sync_time_ns += now_ns() - t0;
    p->profile.sync_count++;
    if (n_outputs && p->out_plan.word_aligned) {
        const char* st = (const char*)p->stage_host;
        uint64_t off = 0;
        for (uint64_t i = 0; i < n_outputs; i++) {
            memcpy(outputs[i].host_ptr, st + off, outputs[i].size);
            off += (outputs[i].size + 3) / 4 * 4;
        }
    }
    return ok;
}

// The decode step's fast path (round 5): inputs, dynamic words, the plan and the outputs as ONE graph launch (zgml_hip_program::
// io_graph). The GPU-side timeline of the copy-command form (profiles/r05_vtable_timeline.txt) shows what the commands around the
// plan's graph cost per token: H2D + wait for the scatter kernel + the kernel, then ~18 us from the last kernel to the D2H's start
// + the copy. Here the scatter kernel reads the pinned staging buffer through its device mapping, the gather kernel writes the
// outputs into a second pinned buffer, and both are nodes of the graph. false: not applicable (no graph, odd alignment, no
// inputs or outputs, profiling) — the caller takes the general path.
static bool execute_io_graph(zgml_hip_ctx* ctx, zgml_hip_program* p, const zgml_program_io* inputs, uint64_t n_inputs,
                             const zgml_program_io* outputs, uint64_t n_outputs, uint64_t t0) {
    if (!sw().hip_io_graph || !ctx->opt_graph || ctx->opt_profile || !n_inputs || !n_outputs || !p->in_plan.word_aligned || !p->out_plan.word_aligned ||
        !p->in_plan.dyn_row || !p->in_plan.table_dev || !p->out_plan.table_dev)
        return false;
    ensure_plan(p);
    if (p->plan.empty()) return false;
    hipStream_t s = ctx->stream;
    { // pack: the inputs, then the dynamic words (always: the graph's scatter launch has a fixed number of rows)
        char* st = (char*)p->stage_host;
        uint64_t off = 0;
        for (uint64_t i = 0; i < n_inputs; i++) {
            memcpy(st + off, inputs[i].host_ptr, inputs[i].size);
            off += (inputs[i].size + 3) / 4 * 4;
        }
        memcpy(st + off, p->dyn_host, p->ops.size() * sizeof(uint32_t));
        p->dyn_dirty = true; // (until the graph that carries them has been launched: a fall-back to the general path must still send them)
    }
    const uint64_t t1 = ctx->host_prof ? now_ns() : 0;
    const uint32_t in_rows = (uint32_t)n_inputs + 1, out_rows = (uint32_t)n_outputs;
    // where the outputs land: the caller's own buffer once it has proved stable (zgml_hip_program::pin_host), else the staging buffer
    if (p->pin_allowed && !p->pin_off && n_outputs == 1) {
        const zgml_program_io& o = outputs[0];
        if (p->pin_host && (p->pin_host != o.host_ptr || p->pin_size != o.size)) { // moved: give the registration up for good
            hipStreamSynchronize(s);
            p->io_graph.reset();
            (void)hipHostUnregister(p->pin_host);
            p->pin_host = p->pin_dev = nullptr, p->pin_off = true;
        } else if (!p->pin_host) {
            p->pin_seen = p->pin_cand == o.host_ptr ? p->pin_seen + 1 : 1;
            p->pin_cand = o.host_ptr;
            if (p->pin_seen >= 3 && o.size >= 4096) {
                void* dev = nullptr;
                if (hipHostRegister(o.host_ptr, o.size, hipHostRegisterMapped) != hipSuccess) { // (e.g. memory the caller has pinned itself: left alone)
                    (void)hipGetLastError();
                    p->pin_off = true;
                } else if (hipHostGetDevicePointer(&dev, o.host_ptr, 0) == hipSuccess && dev) {
                    p->pin_host = o.host_ptr, p->pin_dev = dev, p->pin_size = o.size;
                } else {
                    (void)hipGetLastError();
                    (void)hipHostUnregister(o.host_ptr); // (our own registration)
                    (void)hipGetLastError();
                    p->pin_off = true;
                }
            }
        }
    } else if (p->pin_host) {
        hipStreamSynchronize(s);
        p->io_graph.reset();
        (void)hipHostUnregister(p->pin_host);
        p->pin_host = p->pin_dev = nullptr, p->pin_off = true;
    }
    void* out_dev = p->pin_host ? p->pin_dev : nullptr;
    if (!out_dev && hipHostGetDevicePointer(&out_dev, p->stage_out_host, 0) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    if (p->io_graph.exec && (p->io_in_rows != in_rows || p->io_out_rows != out_rows || p->io_out_dev != out_dev)) p->io_graph.reset();
    if (!p->io_graph.exec) {
        void* in_dev = nullptr;
        if (hipHostGetDevicePointer(&in_dev, p->stage_host, 0) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        const uint32_t gy = io_grid_y(p->out_plan.max_row_words);
        const auto work = [&] {
            scatter_words_kernel<<<dim3(in_rows, io_grid_y(p->in_plan.max_row_words)), 256, 0, s>>>(p->in_plan.table_dev, (const uint32_t*)in_dev);
            run_plan(p, s, 0, p->plan.size());
            gather_words_wide_kernel<<<dim3(out_rows, gy), 256, 0, s>>>(p->out_plan.table_dev, (uint32_t*)out_dev);
        };
        if (!capture_graph(ctx, s, "program-io", work, &p->io_graph)) return false;
        p->io_in_rows = in_rows, p->io_out_rows = out_rows, p->io_out_dev = out_dev;
    }
    if (!CTX_CHECK(ctx, hipGraphLaunch(p->io_graph.exec, s))) return true; // (reported; nothing ran)
    p->dyn_dirty = false;
    const uint64_t t2 = ctx->host_prof ? now_ns() : 0;
    const uint64_t ts = now_ns();
    const bool ok = CTX_CHECK(ctx, hipStreamSynchronize(s)) && ctx->handoff_ok("execute_program");
    p->profile.sync_time_ns += now_ns() - ts;
    p->profile.sync_count++;
    if (ok && !p->pin_host) {
        const char* st = (const char*)p->stage_out_host;
        uint64_t off = 0;
        for (uint64_t i = 0; i < n_outputs; i++) {
            memcpy(outputs[i].host_ptr, st + off, outputs[i].size);
            off += (outputs[i].size + 3) / 4 * 4;
        }
    }
    if (ctx->host_prof) {
        const uint64_t t3 = now_ns();
        ctx->prof_ns[1] += t1 - t0, ctx->prof_ns[2] += t2 - t1, ctx->prof_ns[3] += t3 - t2;
        ctx->prof_calls[1]++, ctx->prof_calls[2]++, ctx->prof_calls[3]++;
    }
    p->profile.call_count++;
    p->profile.backend_op_count += p->ops.size();
    p->profile.backend_dispatch_count += p->plan.size();
    CTX_CHECK(ctx, hipGetLastError());
    return true;
}

int zgml_hip_program_pin_outputs(zgml_hip_ctx* ctx, zgml_hip_program* p, int on) {
    if (!ctx || !p) return -1;
    hipSetDevice(ctx->device);
    if (!on && p->pin_host) {
        hipStreamSynchronize(ctx->stream);
        p->io_graph.reset();
        (void)hipHostUnregister(p->pin_host);
        (void)hipGetLastError();
        p->pin_host = p->pin_dev = nullptr;
    }
    p->pin_allowed = on != 0, p->pin_off = false, p->pin_seen = 0, p->pin_cand = nullptr;
    return 0;
}

void zgml_hip_execute_program(zgml_hip_ctx* ctx, zgml_hip_program* p, const zgml_program_io* inputs, uint64_t n_inputs,
                              const zgml_program_io* outputs, uint64_t n_outputs) {
    if (!ctx || !p) return;
    hipSetDevice(ctx->device);
    // both transfer tables are validated before anything is enqueued
    if (!prepare_io(p, p->in_plan, inputs, n_inputs) || !prepare_io(p, p->out_plan, outputs, n_outputs)) return;
    const uint64_t t0 = ctx->host_prof ? now_ns() : 0;
    if (execute_io_graph(ctx, p, inputs, n_inputs, outputs, n_outputs, t0)) return;
    if (!upload_inputs(ctx, p, inputs, n_inputs)) return;
    const uint64_t t1 = ctx->host_prof ? now_ns() : 0;
    enqueue(p);
    const uint64_t t2 = ctx->host_prof ? now_ns() : 0;
    download_outputs(ctx, p, outputs, n_outputs);
    if (ctx->host_prof) {
        const uint64_t t3 = now_ns();
        ctx->prof_ns[1] += t1 - t0, ctx->prof_ns[2] += t2 - t1, ctx->prof_ns[3] += t3 - t2;
        ctx->prof_calls[1]++, ctx->prof_calls[2]++, ctx->prof_calls[3]++;
    }
    p->profile.call_count++;
    p->profile.backend_op_count += p->ops.size();
    p->profile.backend_dispatch_count += p->plan.size();
    CTX_CHECK(ctx, hipGetLastError());
}

// ── capture-friendly split of a step (multi-GPU harness records ops + collectives into one graph) ──
// stage_inputs: host side only — validate the transfer table and copy the host leaves into the
// pinned staging buffer. enqueue_staged: device side only — one H2D of the staging buffer, the
// scatter kernel and an unconditional copy of the dynamic-parameter block; safe to record into a
// stream capture and replay, the replay picks up whatever stage_inputs / refresh_program wrote last.
int zgml_hip_stage_inputs(zgml_hip_ctx* ctx, zgml_hip_program* p, const zgml_program_io* inputs, uint64_t n_inputs) {
    if (!ctx || !p) return -1;
    hipSetDevice(ctx->device);
    if (!prepare_io(p, p->in_plan, inputs, n_inputs)) return -1;
    if (n_inputs && !p->in_plan.word_aligned) {
        ctx->fail("stage_inputs: inputs must be 4-byte aligned in offset and size");
        return -1;
    }
    char* st = (char*)p->stage_host;
    uint64_t off = 0;
    for (uint64_t i = 0; i < n_inputs; i++) {
        memcpy(st + off, inputs[i].host_ptr, inputs[i].size);
        off += (inputs[i].size + 3) / 4 * 4;
    }
    p->staged_bytes = off;
    p->staged_n = n_inputs;
    return 0;
}

void zgml_hip_enqueue_staged(zgml_hip_ctx* ctx, zgml_hip_program* p) {
    if (!ctx || !p) return;
    hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    if (p->staged_n) {
        hipMemcpyAsync(p->stage_dev, p->stage_host, p->staged_bytes, hipMemcpyHostToDevice, s);
        scatter_words_kernel<<<dim3((uint32_t)p->staged_n, io_grid_y(p->in_plan.max_row_words)), 256, 0, s>>>(p->in_plan.table_dev, (const uint32_t*)p->stage_dev);
    }
    if (!p->ops.empty()) hipMemcpyAsync(p->dyn_dev, p->dyn_host, p->ops.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s);
    p->dyn_dirty = false;
}

// argmax without the blocking read-back: result lands in pinned memory, read it with
// zgml_hip_argmax_result after synchronising the stream (or after a graph replay completed)
int zgml_hip_enqueue_argmax(zgml_hip_ctx* ctx, zgml_hip_program* p, uint16_t buf_idx, uint64_t offset, uint64_t n) {
    if (!ctx || !p || buf_idx >= p->bufs.size() || !p->bufs[buf_idx] || offset + n > p->sizes[buf_idx]) return -1;
    hipSetDevice(ctx->device);
    launch_argmax(ctx->stream, p->bufs[buf_idx] + offset, n, ctx->arg_val, ctx->arg_idx, ctx->arg_out);
    hipMemcpyAsync(ctx->arg_out_host, ctx->arg_out, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream);
    return 0;
}
int64_t zgml_hip_argmax_result(zgml_hip_ctx* ctx) { return ctx ? *ctx->arg_out_host : -1; }

void zgml_hip_upload_inputs(zgml_hip_ctx* ctx, zgml_hip_program* p, const zgml_program_io* inputs, uint64_t n_inputs) {
    if (!ctx || !p) return;
    hipSetDevice(ctx->device);
    upload_inputs(ctx, p, inputs, n_inputs);
}

void zgml_hip_download_outputs(zgml_hip_ctx* ctx, zgml_hip_program* p, const zgml_program_io* outputs, uint64_t n_outputs) {
    if (!ctx || !p) return;
    hipSetDevice(ctx->device);
    download_outputs(ctx, p, outputs, n_outputs);
}

void shard_peer_release(zgml_hip_program* p); // (runtime_shard.hip)
void zgml_hip_free_program(zgml_hip_ctx* ctx, zgml_hip_program* p) {
    if (!p) return;
    if (ctx) {
        hipSetDevice(ctx->device);
        hipStreamSynchronize(ctx->stream);
    }
    if (ctx && !ctx->handoff_ok("free_program")) fprintf(stderr, "[zgml_hip] ERROR: %s\n", ctx->err.c_str());
    for (void* d : p->fuse_owned) hipFree(d);
    if (!p->attn_traces.empty()) { // stamps of the last execution, 100 MHz wall clock -> ns
        fprintf(stderr, "[zgml_hip] attention trace (ns since previous launch's end | start->params | ->dyn | ->rope | ->scores | ->max | ->pv | ->end)\n");
        unsigned long long prev_end = 0;
        for (size_t i = 0; i < p->attn_traces.size(); i++) {
            const unsigned long long* t = p->attn_traces[i];
            fprintf(stderr, "  L%02zu gap %6lld |", i, prev_end ? (long long)(t[0] - prev_end) * 10 : -1);
            for (int k = 1; k < 8; k++) fprintf(stderr, " %5lld", (long long)(t[k] - t[k - 1]) * 10);
            if (t[8]) fprintf(stderr, " | sweeps %3llu first-rtt %5llu", t[8], t[9] * 10); // (the granule hand-off's wait: attention_decode.h)
            fprintf(stderr, "\n");
            prev_end = t[7];
        }
        for (auto* t : p->attn_traces) hipHostFree(t);
    }
    if (!p->xcc_traces.empty()) { // of the last execution: how many (projection column group, consuming head) pairs shared an XCD
        uint64_t pairs0 = 0, same0 = 0, pairs_n = 0, same_n = 0;
        for (const auto& x : p->xcc_traces) {
            const uint32_t pk = x.d_head / 16, hpg = x.n_heads / x.n_kv, nq = x.n_heads * pk, nk = x.n_kv * pk;
            for (uint32_t r = 0; r < x.n_heads; r++) // (recorded only where record r is a head of kv group r / hpg: fuse_qkv_attention)
                for (uint32_t sp = 0; sp < x.n_sp; sp++) {
                    const uint32_t c = x.w[x.n_mv + r * x.n_sp + sp];
                    if (!c) continue; // an idle split
                    for (uint32_t i = 0; i < 3 * pk; i++) {
                        const uint32_t part = i / pk, g = i % pk, cg = part == 0 ? r * pk + g : nq + (part - 1) * nk + (r / hpg) * pk + g;
                        if (!x.w[cg]) continue;
                        (sp ? pairs_n : pairs0)++;
                        if (x.w[cg] == c) (sp ? same_n : same0)++;
                    }
                }
        }
        fprintf(stderr, "[zgml_hip] fused q/k/v + attention, %zu launches: producer / consumer pairs on one XCD: split 0 %llu of %llu, splits >= 1 %llu of %llu\n",
                p->xcc_traces.size(), (unsigned long long)same0, (unsigned long long)pairs0, (unsigned long long)same_n, (unsigned long long)pairs_n);
        for (const auto& x : p->xcc_traces) hipHostFree(x.w);
    }
    if (!p->ks_traces.empty()) {
        fprintf(stderr, "[zgml_hip] K-split launches, workgroup 0, ns between stamps (gap = since the previous launch's last stamp); ks-proj / ks-mlp: start | loads issued | "
                        "parts summed | vector whole | x staged | FMAs | barrier | folded (mlp: + SiLU) | (mlp: barrier | down partial); ks-attn-o: start | record | loads issued | attention | merged | partial O\n");
        unsigned long long prev_end = 0;
        for (const auto& k : p->ks_traces) {
            int last = 0;
            for (int j = 0; j < 16; j++)
                if (k.t[j]) last = j;
            fprintf(stderr, "  %-10s gap %6lld |", k.what, prev_end ? (long long)(k.t[0] - prev_end) * 10 : -1);
            for (int j = 1; j <= last; j++) fprintf(stderr, " %5lld", k.t[j] ? (long long)(k.t[j] - k.t[j - 1]) * 10 : -1);
            fprintf(stderr, " | span %5lld\n", (long long)(k.t[last] - k.t[0]) * 10);
            if (k.t[16]) { // lane 0 of the workgroup's last wave: its stamps relative to thread 0's start
                fprintf(stderr, "      last wave: start %+5lld |", (long long)(k.t[16] - k.t[0]) * 10);
                for (int j = 1; j <= last && j < 12; j++) fprintf(stderr, " %5lld", k.t[16 + j] ? (long long)(k.t[16 + j] - k.t[16 + j - 1]) * 10 : -1);
                fprintf(stderr, "\n");
            }
            prev_end = k.t[last];
        }
        for (auto& k : p->ks_traces) hipHostFree(k.t);
    }
    if (!p->qmv_traces.empty()) {
        fprintf(stderr, "[zgml_hip] mat-vec trace, workgroup 0 (ns: gap since previous mat-vec end | ->loads issued | ->x arrived(+sumsq) | ->x staged | ->streamed | ->reduced+epilogue)"
                        " || K-on-lanes launches also: LAST workgroup, start after workgroup 0's start | ->loads issued | ->streamed | ->end; launch span = first start -> last end\n");
        unsigned long long prev_end = 0;
        for (size_t i = 0; i < p->qmv_traces.size() && i < 48; i++) {
            const auto& q = p->qmv_traces[i];
            fprintf(stderr, "  #%02zu K=%5u N0=%5u parts=%u pro=%u gap %6lld |", i, q.K, q.N, q.parts, q.pro,
                    prev_end ? (long long)(q.t[0] - prev_end) * 10 : -1);
            for (int k = 1; k < 6; k++) fprintf(stderr, " %5lld", (long long)(q.t[k] - q.t[k - 1]) * 10);
            if (q.t[8]) {
                fprintf(stderr, " || %5lld | %5lld %5lld %5lld | span %5lld", (long long)(q.t[8] - q.t[0]) * 10, (long long)(q.t[9] - q.t[8]) * 10,
                        (long long)(q.t[12] - q.t[9]) * 10, (long long)(q.t[13] - q.t[12]) * 10, (long long)(std::max(q.t[13], q.t[5]) - q.t[0]) * 10);
                prev_end = std::max(q.t[13], q.t[5]);
            } else {
                prev_end = q.t[5];
            }
            fprintf(stderr, "\n");
        }
        for (auto& q : p->qmv_traces) hipHostFree(q.t);
    }
    free_graph(p);
    free_resident(p);
    free_param_blobs(p);
    shard_peer_release(p);
    if (p->arena) hipFree(p->arena);
    if (p->zero_word) hipFree(p->zero_word);
    for (void* d : p->owned) hipFree(d);
    if (p->scratch) hipFree((char*)p->scratch - kQmmScratchHead);
    if (p->dyn_dev) hipFree(p->dyn_dev);
    if (p->dyn_host) hipHostFree(p->dyn_host);
    if (p->pin_host) (void)hipHostUnregister(p->pin_host), (void)hipGetLastError();
    if (p->stage_host) hipHostFree(p->stage_host);
    if (p->stage_out_host) hipHostFree(p->stage_out_host);
    if (p->stage_dev) hipFree(p->stage_dev);
    if (p->in_plan.table_dev) hipFree(p->in_plan.table_dev);
    if (p->out_plan.table_dev) hipFree(p->out_plan.table_dev);
    delete p;
}

zgml_runtime_profile* zgml_hip_get_runtime_profile(zgml_hip_ctx*, zgml_hip_program* p) {
    return p ? &p->profile : nullptr;
}

// ── extensions ──────────────────────────────────────────────────────────────────────────────

uint64_t zgml_hip_program_plan_text(zgml_hip_ctx* ctx, zgml_hip_program* p, char* out, uint64_t cap) {
    if (!ctx || !p) return 0;
    ensure_plan(p);
    static const char* const pro_names[4] = {"none", "mul", "rmsnorm", "prenorm"};
    std::string t;
    for (size_t i = 0; i < p->plan.size(); i++) {
        const Launch& L = p->plan[i];
        char line[256];
        snprintf(line, sizeof line, "%zu: kind %u ops %u [%u..%u]", i, L.kind, L.n_ops, L.op_lo, L.op_hi);
        t += line;
        if (L.qmv_desc) {
            const QmvLaunch& q = *L.qmv_desc;
            snprintf(line, sizeof line, " qmv parts %u K %u pro %s%s%s", q.n_parts, q.K, pro_names[q.pro.kind < 4 ? q.pro.kind : 0], q.next.xg_out ? " prepares-next-norm" : "",
                     q.pair_out ? " pair" : "");
            t += line;
        }
        if (L.adec_desc) { // the head records the launch carries, and their form (kvq: int8 KV caches)
            snprintf(line, sizeof line, "%s heads %u%s", L.qmv_desc ? " +decode-attention" : " decode-attention", L.adec_desc->nh, L.adec_desc->kvq ? " kvq" : "");
            t += line;
        }
        if (L.tag) t += std::string(" ") + L.tag;
        if (L.hook && L.hook->ap && *L.hook->ap) t += " writes-A-operand";
        t += "\n";
    }
    if (out && cap) {
        const uint64_t n = std::min<uint64_t>(cap - 1, t.size());
        memcpy(out, t.data(), n);
        out[n] = 0;
    }
    return t.size();
}

void* zgml_hip_program_buffer_ptr(zgml_hip_program* p, uint16_t buf_idx) {
    if (p) unhoist_if_guarded(p, buf_idx);
    return (p && buf_idx < p->bufs.size()) ? p->bufs[buf_idx] : nullptr;
}

void* zgml_hip_stream(zgml_hip_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

void zgml_hip_enqueue_program(zgml_hip_ctx* ctx, zgml_hip_program* p) {
    if (!ctx || !p) return;
    hipSetDevice(ctx->device);
    enqueue(p);
}

int zgml_hip_copy_program_buffer(zgml_hip_ctx* ctx, zgml_hip_program* dst, uint16_t dst_buf, uint64_t dst_offset,
                                 zgml_hip_program* src, uint16_t src_buf, uint64_t src_offset, uint64_t n_elems) {
    if (!ctx || !dst || !src) return -1;
    if (dst_buf >= dst->bufs.size() || src_buf >= src->bufs.size() || !dst->bufs[dst_buf] || !src->bufs[src_buf]) {
        ctx->fail("copy_program_buffer: no such live buffer");
        return -1;
    }
    if (dst_offset + n_elems > dst->sizes[dst_buf] || src_offset + n_elems > src->sizes[src_buf]) {
        ctx->fail("copy_program_buffer: range exceeds a buffer");
        return -1;
    }
    unhoist_if_guarded(dst, dst_buf);
    hipSetDevice(ctx->device);
    return CTX_CHECK(ctx, hipMemcpyAsync(dst->bufs[dst_buf] + dst_offset, src->bufs[src_buf] + src_offset, n_elems * sizeof(float),
                                         hipMemcpyDeviceToDevice, ctx->stream))
               ? 0
               : -1;
}

void zgml_hip_enqueue_ops(zgml_hip_ctx* ctx, zgml_hip_program* p, uint64_t first, uint64_t count) {
    if (!ctx || !p) return;
    hipSetDevice(ctx->device);
    if (!p->ksplit_off && !(first == 0 && count >= p->ops.size())) // an op range must leave every buffer written: no deferred vectors in this program's plans
        p->ksplit_off = true, p->plan_dirty = p->plan_dirty || p->has_deferred;
    ensure_plan(p);
    flush_dyn(p);
    // a launch belongs to the range when every op it covers does; barriers (set_barriers) make
    // sure batching never straddles the harness's collective points
    for (auto& L : p->plan) {
        if (L.op_lo >= first && L.op_hi < first + count) {
            L.run(ctx->stream);
        } else if (!(L.op_hi < first || L.op_lo >= first + count)) {
            ctx->fail("enqueue_ops: range cuts through a batched launch; declare it with zgml_hip_program_set_barriers");
            return;
        }
    }
}

int zgml_hip_program_set_barriers(zgml_hip_ctx* ctx, zgml_hip_program* p, const uint64_t* op_indices, uint64_t n) {
    if (!ctx || !p) return -1;
    p->barriers.assign(op_indices, op_indices + n);
    std::sort(p->barriers.begin(), p->barriers.end());
    p->plan_dirty = true;
    return 0;
}

void zgml_hip_synchronize(zgml_hip_ctx* ctx) {
    if (!ctx) return;
    if (CTX_CHECK(ctx, hipStreamSynchronize(ctx->stream))) ctx->handoff_ok("synchronize");
}

int64_t zgml_hip_argmax(zgml_hip_ctx* ctx, zgml_hip_program* p, uint16_t buf_idx, uint64_t offset, uint64_t n) {
    if (!ctx || !p || buf_idx >= p->bufs.size() || !p->bufs[buf_idx] || offset + n > p->sizes[buf_idx]) return -1;
    hipSetDevice(ctx->device);
    launch_argmax(ctx->stream, p->bufs[buf_idx] + offset, n, ctx->arg_val, ctx->arg_idx, ctx->arg_out);
    hipMemcpyAsync(ctx->arg_out_host, ctx->arg_out, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream);
    if (!CTX_CHECK(ctx, hipStreamSynchronize(ctx->stream)) || !ctx->handoff_ok("argmax")) return -1;
    return *ctx->arg_out_host;
}

} // extern "C"
