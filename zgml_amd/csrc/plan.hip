// plan.hip — the launch planner: everything that turns a program's ops (p->ops) into its launch list (p->plan). Host code only:
// the launches run the kernels of the other translation units (kernels.h).
#include "runtime_internal.h"

namespace {

// ── plan building ───────────────────────────────────────────────────────────────────────────
// Serial mode: one launch per DeviceOp in program order. Batched mode (ZGML_HIP_OPT_FUSION, the
// default): ops are grouped by dependency level (schedule.h); inside a level every rope /
// slice_assign / attention / repeat goes into ONE launch of its kind (parameters in a device
// array, blockIdx.y = op), the rest launch one by one.
float* buf_at(zgml_hip_program* p, uint16_t idx, uint64_t off) { return p->bufs[idx] + off; }

template <typename T>
const T* upload_params(zgml_hip_program* p, const std::vector<T>& v) {
    void* d = nullptr;
    if (hipMalloc(&d, v.size() * sizeof(T)) != hipSuccess) {
        p->ctx->fail("plan: parameter array allocation failed");
        return nullptr;
    }
    if (h2d_sync(p->ctx->stream, d, v.data(), v.size() * sizeof(T)) != hipSuccess) p->ctx->fail("plan: parameter array upload failed");
    p->param_blobs.push_back(d);
    return (const T*)d;
}

// Split policy of one decode-attention launch (kernels.h AttnSplit): up to 16 workgroups per head, one
// per `min_keys` keys of the longest context the plan allows, the whole launch within ~256 workgroups.
// ZGML_HIP_OPT_ATTN_SPLIT_MIN_KEYS (or the ZGML_HIP_ATTN_SPLIT_MIN_KEYS environment variable) moves the
// threshold (>= 32, 0 = off); ZGML_HIP_ATTN_SPLIT caps the workgroups per head (<= 1 = off).
// `default_min_keys`: 128 — except where a workgroup covers few keys per memory round trip: the 4-wave form of the f32-KV decode
// attention at d_head 128 (stand-alone and inside the K-on-lanes fused launch) streams 32 keys per round, so a head waits four
// dependent rounds per 128 keys; splitting from 64 keys on gave Llama-2-7B +4 % over positions 200..328 (760 -> 791 tok/s) at no
// cost at positions 4..132 and 1900 (profiles/r05_split_sweep_7b.txt; 32 is worse again: the merge costs more than a round).
AttnSplit attn_split_for(zgml_hip_program* p, uint32_t n_heads, uint32_t d_head, uint32_t max_kv, int default_min_keys = 128) {
    const int want = sw().hip_attn_split;
    const int min_keys_env = sw().hip_attn_split_min_keys;
    AttnSplit sp;
    const int64_t min_keys = p->ctx->opt_attn_split_min_keys >= 0 ? p->ctx->opt_attn_split_min_keys : (min_keys_env >= 0 ? min_keys_env : default_min_keys);
    if (min_keys == 0 || want <= 1) return sp;
    sp.min_keys = (uint32_t)std::min<int64_t>(std::max<int64_t>(32, min_keys), 1 << 30);
    uint32_t S = std::min<uint32_t>((uint32_t)std::max(want, 1), max_kv / sp.min_keys);
    S = std::min(S, std::max(1u, (uint32_t)sw().hip_attn_split_wgs / std::max(n_heads, 1u))); // about one (1024-thread) workgroup per CU: idle ones still cost dispatch
    if (S <= 1) return sp;
    const uint64_t need = (uint64_t)n_heads * S * (d_head + 4);
    if (need > p->split_buf_floats) { // earlier launches keep their (smaller) block: it stays in param_blobs
        void* d = nullptr;
        if (hipMalloc(&d, need * sizeof(float)) != hipSuccess) return sp;
        p->param_blobs.push_back(d);
        p->split_buf = (float*)d, p->split_buf_floats = need;
    }
    if (n_heads > p->split_cnt_words) {
        void* d = nullptr;
        const size_t bytes = ((size_t)n_heads * 4 + 255) / 256 * 256;
        if (hipMalloc(&d, bytes) != hipSuccess || memset_sync(p->ctx->stream, d, 0, bytes) != hipSuccess) return sp;
        p->param_blobs.push_back(d);
        p->split_cnt = (uint32_t*)d, p->split_cnt_words = n_heads;
    }
    sp.splits = S, sp.buf = p->split_buf, sp.cnt = p->split_cnt;
    return sp;
}

RepeatParams make_repeat(zgml_hip_program* p, const zgml_op_repeat& r) {
    RepeatParams rp{};
    rp.dst = p->bufs[r.dst];
    rp.src = p->bufs[r.src];
    rp.n = r.n;
    for (int d = 0; d < 4; d++) {
        rp.src_ne[d] = r.src_ne[d] ? r.src_ne[d] : 1;
        rp.src_strides[d] = r.src_strides[d];
        rp.dst_strides[d] = r.dst_strides[d] ? r.dst_strides[d] : 1;
    }
    rp.src_offset = r.src_offset, rp.dst_offset = r.dst_offset;
    const uint64_t src_n = (uint64_t)r.src_ne[0] * r.src_ne[1] * r.src_ne[2] * r.src_ne[3];
    rp.src_n = (uint32_t)src_n;
    // the reference's fast paths (reference.zig:401-419), in its order of precedence
    if (src_n == 1)
        rp.mode = 1;
    else if (src_n >= r.n)
        rp.mode = 2;
    else if (r.n % src_n == 0 && r.src_strides[0] == 1 && (r.src_ne[1] <= 1 || r.src_strides[1] == r.src_ne[0]) &&
             (r.src_ne[2] <= 1 || r.src_strides[2] == r.src_ne[0] * r.src_ne[1]) &&
             (r.src_ne[3] <= 1 || r.src_strides[3] == r.src_ne[0] * r.src_ne[1] * r.src_ne[2]))
        rp.mode = 3;
    else
        rp.mode = 0;
    return rp;
}

SliceAssignParams make_slice_assign(zgml_hip_program* p, const zgml_op_slice_assign& sa, size_t op_index) {
    SliceAssignParams sp{};
    sp.dst = p->bufs[sa.dst];
    sp.src = buf_at(p, sa.src, sa.src_offset);
    sp.rows = sa.rows, sp.cols = sa.cols;
    sp.dst_row_stride = sa.dst_row_stride, sp.dst_col_stride = sa.dst_col_stride;
    sp.src_row_stride = sa.src_row_stride, sp.src_col_stride = sa.src_col_stride;
    sp.dyn_dst_offset = p->dyn_dev + op_index;
    return sp;
}

RopeParams make_rope(zgml_hip_program* p, const zgml_op_rope& r) {
    RopeParams rp{};
    rp.dst = buf_at(p, r.dst, r.dst_off);
    rp.src = buf_at(p, r.src, r.src_off);
    rp.cs = buf_at(p, r.cos_sin, r.cs_off);
    rp.half_d = r.half_d, rp.seq_len = r.seq_len, rp.src_rs = r.src_rs, rp.src_cs = r.src_cs, rp.cs_cs = r.cs_cs;
    rp.dst2 = nullptr, rp.dyn_dst2_off = nullptr, rp.d2_rs = rp.d2_cs = 0;
    return rp;
}

AttentionParams make_attention(zgml_hip_program* p, const zgml_op_attention& a, size_t op_index) {
    AttentionParams ap{};
    ap.dst = buf_at(p, a.dst, a.dst_off);
    ap.q = buf_at(p, a.q, a.q_off);
    ap.k = buf_at(p, a.k, a.k_off);
    ap.v = buf_at(p, a.v, a.v_off);
    ap.mask = a.has_mask ? buf_at(p, a.mask, a.mask_off) : nullptr;
    ap.d_head = a.d_head, ap.seq_q = a.seq_q;
    ap.dyn_seq_kv = p->dyn_dev + op_index;
    ap.scale = a.scale;
    ap.q_rs = a.q_rs, ap.q_cs = a.q_cs, ap.k_rs = a.k_rs, ap.k_cs = a.k_cs, ap.v_rs = a.v_rs, ap.v_cs = a.v_cs;
    ap.mask_rs = a.mask_rs, ap.mask_cs = a.mask_cs, ap.dst_rs = a.dst_rs, ap.dst_cs = a.dst_cs;
    ap.dst2 = nullptr, ap.dyn_dst2_off = nullptr, ap.d2_rs = ap.d2_cs = 0;
    return ap;
}

// The A-operand hand-over (SplitHook): true when an op behind the producing launch's last member and in front of op i (program
// order) writes into the rows the matmul at op i reads — a slice_assign, an in-place elementwise or softmax, another chain over
// a different extent. The operand that launch would emit is then stale by the time the matmul runs: the matmul prepares its own.
// (Spans as the schedule assumes them: a dynamic store counts with its whole slab. Hooks exist in batched plans only.)
bool rows_rewritten_after(const zgml_hip_program* p, const Launch& producer, size_t i, const Span& rows) {
    for (size_t j = (size_t)producer.op_hi + 1; j < i && j < p->sched.access.size(); j++)
        for (const Span& w : p->sched.access[j].writes)
            if (spans_overlap(w, rows)) return true;
    return false;
}

// launch for a single op of a kind that is never batched
bool make_single(zgml_hip_program* p, size_t i, Launch& L) {
    const zgml_device_op& op = p->ops[i];
    L.kind = op.kind, L.n_ops = 1, L.op_lo = L.op_hi = (uint32_t)i;
    switch (op.kind) {
        case ZGML_DOP_ELEMENTWISE: {
            const auto e = op.u.elementwise;
            float* dst = buf_at(p, e.dst, e.dst_offset);
            const float* s0 = buf_at(p, e.src0, e.src0_offset);
            const float* s1 = buf_at(p, e.src1, e.src1_offset);
            L.run = [=](hipStream_t s) { launch_elementwise(s, e.op, dst, s0, s1, e.n); };
            return true;
        }
        case ZGML_DOP_MATMUL: {
            const auto m = op.u.matmul;
            DenseMatmulParams dp{};
            dp.dst = buf_at(p, m.dst, m.geom.dst_offset);
            dp.a = buf_at(p, m.a, m.geom.a_offset);
            dp.b = buf_at(p, m.b, m.geom.b_offset);
            dp.M = (uint32_t)m.geom.M, dp.N = (uint32_t)m.geom.N, dp.K = (uint32_t)m.geom.K;
            dp.a_rs = (uint32_t)m.geom.a_row_stride, dp.a_cs = (uint32_t)m.geom.a_col_stride;
            dp.b_rs = (uint32_t)m.geom.b_row_stride, dp.b_cs = (uint32_t)m.geom.b_col_stride;
            dp.dst_rs = (uint32_t)m.geom.dst_row_stride;
            dp.b_f16 = 0;
            if (m.b < p->f16_weights.size() && p->f16_weights[m.b]) { // promoted at compile time
                DenseF16Params fp{dp.dst, dp.a, p->f16_weights[m.b], dp.M, dp.N, dp.K, dp.a_rs, dp.dst_rs, p->f16_stream_nt ? 1u : 0u};
                if (p->scratch && dense_f16_scratch_bytes(dp.M, dp.K)) { // same adjacency rule as the quantized split below
                    const uint64_t pos = p->plan.size();
                    fp.scratch = p->scratch;
                    fp.reuse_a = p->split_pos + 1 == pos && p->split_input == dp.a && p->split_M == dp.M && p->split_K == dp.K &&
                                 p->split_in_rs == dp.a_rs && p->split_kind == 2;
                    const bool adjacent = fp.reuse_a; // the launch at split_pos is the plan's last one: only that one can be joined
                    // ... or the launch that produced the rows wrote the operand itself (as for the quantized split below)
                    if (!fp.reuse_a && sw().hip_fuse_split && dense_f16_a_unpadded(dp.M, dp.K) && dp.a_rs == dp.K) {
                        for (size_t back = p->plan.size(); back-- > 0;) {
                            const Launch& prev = p->plan[back];
                            const bool fits = prev.hook && prev.hook->out == dp.a &&
                                              (prev.hook->rows ? prev.hook->rows == dp.M && prev.hook->cols == dp.K : (uint64_t)dp.M * dp.K == prev.hook->n);
                            if (fits) {
                                if (rows_rewritten_after(p, prev, i, Span{m.a, m.geom.a_offset, m.geom.a_offset + (uint64_t)dp.M * dp.K})) break;
                                *prev.hook->ap = (uint16_t*)p->scratch, *prev.hook->ap_S = kApF16 | (dp.K / 32);
                                if (prev.hook->ap_cols) *prev.hook->ap_cols = dp.K;
                                fp.reuse_a = 1;
                                break;
                            }
                            if (prev.kind == ZGML_DOP_QMATMUL || prev.kind == ZGML_DOP_MATMUL) break; // may own the scratch
                        }
                    }
                    p->split_pos = pos, p->split_input = dp.a, p->split_M = dp.M, p->split_K = dp.K, p->split_in_rs = dp.a_rs, p->split_kind = 2;
                    bool joins = adjacent && p->f16_group && p->f16_group->size() < dense_f16_max_group();
                    for (size_t t = 0; joins && t < p->f16_group->size(); t++) joins = dense_f16_can_group((*p->f16_group)[t], fp);
                    if (joins) { // same rows, same K (q/k/v, gate/up): one launch
                        p->f16_group->push_back(fp);
                        Launch& prev = p->plan.back();
                        prev.n_ops++, prev.op_hi = (uint32_t)i;
                        p->split_pos = pos - 1;
                        return false;
                    }
                    auto group = std::make_shared<std::vector<DenseF16Params>>();
                    group->push_back(fp);
                    p->f16_group = group;
                    L.run = [=](hipStream_t s) { launch_dense_f16_group(s, group->data(), (uint32_t)group->size()); };
                    return true;
                }
                L.run = [=](hipStream_t s) { launch_dense_f16(s, fp); };
                return true;
            }
            L.run = [=](hipStream_t s) { launch_dense_matmul(s, dp); };
            L.run_tail = [=](hipStream_t s, DenseHeadTail* tail) { launch_dense_matmul(s, dp, tail); };
            return true;
        }
        case ZGML_DOP_QMATMUL: {
            const auto q = op.u.qmatmul;
            QMatmulParams qp{};
            qp.dst = buf_at(p, q.dst, q.dst_offset);
            qp.input = buf_at(p, q.input, q.input_offset);
            qp.M = q.M, qp.N = q.N, qp.K = q.K;
            qp.in_rs = q.input_row_stride ? q.input_row_stride : q.K;
            qp.dst_rs = q.dst_row_stride ? q.dst_row_stride : q.N;
            const QWeightDev w = p->qweights[q.weight_idx];
            float* scratch = p->scratch;
            // q/k/v and gate/up read the same rows: the launch right after one that split the same input
            // (adjacent in the plan, so nothing rewrote the rows or the scratch in between) reuses its A pieces
            const uint64_t pos = p->plan.size();
            const bool splits = scratch && qmatmul_scratch_bytes(w, qp.M) != 0;
            qp.reuse_split = splits && p->split_pos + 1 == pos && p->split_input == qp.input && p->split_M == qp.M && p->split_K == qp.K &&
                             p->split_in_rs == qp.in_rs && p->split_kind == 1;
            // (a matmul armed through a producer's hook below starts a group of its own: the producer's launch stands between it
            // and the launch at split_pos, which ran before the producer rewrote the rows)
            const bool adjacent = qp.reuse_split;
            // ... or finds them written by the launch that produced the rows (a row chain, an elementwise chain or the attention
            // tile kernel in front of it; no other splitting launch in between, and no op that rewrites the rows after the
            // producer's last member: rows_rewritten_after): that launch is armed and this one skips its split_a_kernel launch
            if (splits && !qp.reuse_split && sw().hip_fuse_split && qp.M % 16 == 0 && qp.K % 128 == 0 && qp.in_rs == qp.K) {
                for (size_t back = p->plan.size(); back-- > 0;) {
                    const Launch& prev = p->plan[back];
                    const bool fits = prev.hook && prev.hook->out == qp.input &&
                                      (prev.hook->rows ? prev.hook->rows == qp.M && prev.hook->cols == qp.K : (uint64_t)qp.M * qp.K == prev.hook->n);
                    if (fits) {
                        if (rows_rewritten_after(p, prev, i, Span{q.input, q.input_offset, q.input_offset + (uint64_t)qp.M * qp.K})) break;
                        *prev.hook->ap = (uint16_t*)scratch, *prev.hook->ap_S = qp.K / 128;
                        if (prev.hook->ap_cols) *prev.hook->ap_cols = qp.K;
                        qp.reuse_split = 1;
                        if (sw().hip_debug_plan.set) fprintf(stderr, "[zgml_hip] A pieces of op %u (M %u, K %u) written by the launch of kind %u at plan[%zu]\n", (unsigned)i, qp.M, qp.K, prev.kind, back);
                        break;
                    }
                    if (prev.kind == ZGML_DOP_QMATMUL || prev.kind == ZGML_DOP_MATMUL) break; // may own the scratch
                }
            }
            if (splits)
                p->split_pos = pos, p->split_input = qp.input, p->split_M = qp.M, p->split_K = qp.K, p->split_in_rs = qp.in_rs, p->split_kind = 1;
            // ... and joins its launch when the kernel can take another part (same rows, same K: q/k/v, gate/up)
            bool joins = adjacent && p->qmm_group && p->qmm_group->size() < qmatmul_max_group();
            for (size_t t = 0; joins && t < p->qmm_group->size(); t++) joins = qmatmul_can_group((*p->qmm_group)[t].first, (*p->qmm_group)[t].second, w, qp);
            if (joins) {
                p->qmm_group->push_back({w, qp});
                Launch& prev = p->plan.back();
                prev.n_ops++, prev.op_hi = (uint32_t)i;
                p->split_pos = pos - 1; // the merged launch still sits at the previous plan position
                return false;
            }
            if (w.format == QW_Q4K && qp.M >= 2 && qp.M <= p->kon_max_m) L.tag = "qmatvec-kon-rows"; // (launch_qmatmul: the multi-row K-on-lanes mat-vec)
            auto group = std::make_shared<std::vector<std::pair<QWeightDev, QMatmulParams>>>();
            group->push_back({w, qp});
            p->qmm_group = splits ? group : nullptr;
            L.run = [=](hipStream_t s) {
                QWeightDev ws[4];
                QMatmulParams ps[4];
                const uint32_t n = (uint32_t)group->size();
                for (uint32_t t = 0; t < n; t++) ws[t] = (*group)[t].first, ps[t] = (*group)[t].second;
                launch_qmatmul_group(s, ws, ps, n, scratch);
            };
            return true;
        }
        case ZGML_DOP_SOFTMAX:
        case ZGML_DOP_LAYERNORM:
        case ZGML_DOP_RMSNORM: {
            const auto r = op.u.rmsnorm;
            float* dst = buf_at(p, r.dst, r.dst_offset);
            const float* src = buf_at(p, r.src, r.src_offset);
            const uint32_t kind = op.kind;
            L.run = [=](hipStream_t s) {
                if (kind == ZGML_DOP_SOFTMAX)
                    launch_softmax(s, dst, src, r.rows, r.cols);
                else if (kind == ZGML_DOP_LAYERNORM)
                    launch_layernorm(s, dst, src, r.rows, r.cols, r.eps);
                else
                    launch_rmsnorm(s, dst, src, r.rows, r.cols, r.eps);
            };
            return true;
        }
        case ZGML_DOP_REDUCE: {
            const auto r = op.u.reduce;
            float* dst = buf_at(p, r.dst, r.dst_offset);
            const float* src = buf_at(p, r.src, r.src_offset);
            L.run = [=](hipStream_t s) { launch_reduce(s, r.op, dst, src, r.n_out, r.reduce_size); };
            return true;
        }
        case ZGML_DOP_FUSED_ELEMENTWISE: {
            const auto fe = op.u.fused_elementwise;
            FusedParams fp{};
            fp.dst = buf_at(p, fe.dst, fe.dst_offset);
            fp.src = buf_at(p, fe.src, fe.src_offset);
            fp.n = fe.n;
            fp.n_steps = fe.n_steps;
            for (uint32_t s = 0; s < fe.n_steps; s++) {
                fp.steps[s].op = fe.steps[s].op;
                fp.steps[s].swapped = fe.steps[s].is_swapped;
                const bool bin = fe.steps[s].op == ZGML_OP_ADD || fe.steps[s].op == ZGML_OP_MUL;
                fp.steps[s].secondary = bin ? buf_at(p, fe.steps[s].secondary_buf, fe.steps[s].secondary_offset) : nullptr;
            }
            L.run = [=](hipStream_t s) { launch_fused_elementwise(s, fp); };
            return true;
        }
        default: return false;
    }
}

// One schedulable item: an op, optionally with the slice_assign that was folded into it
// (rope -> KV store, attention -> row store).
struct PlanItem {
    uint32_t op;
    int store = -1;
};

// the layout the float4-per-lane attention kernels (dense, rows, tiles) read: unit row strides, d_head a power of two in
// [4, 256], column strides in whole float4s and 16-byte aligned q / k / v rows. Anything else runs attention_kernel.
bool attention_op_dense(const AttentionParams& a) {
    const uint32_t dh = a.d_head;
    return a.q_rs == 1 && a.k_rs == 1 && a.v_rs == 1 && dh >= 4 && dh <= 256 && (dh & (dh - 1)) == 0 && (a.q_cs % 4) == 0 &&
           (a.k_cs % 4) == 0 && (a.v_cs % 4) == 0 && ((uintptr_t)a.q % 16) == 0 && ((uintptr_t)a.k % 16) == 0 && ((uintptr_t)a.v % 16) == 0;
}

// the batchable kinds of one group of mutually independent items -> one "movement" launch (ropes
// and slice_assigns together), one attention launch, one repeat launch; the rest one by one
void emit_batches(zgml_hip_program* p, const std::vector<PlanItem>& group) {
    std::vector<RepeatParams> reps, hoisted;
    uint32_t hoisted_max = 0;
    std::vector<MoveParams> moves;
    std::vector<AttentionParams> atts;
    std::vector<int64_t> att_store_off; // per attention: the static offset of its folded row store (else -1)
    std::vector<KvqStoreParams> kstores;
    std::map<uint32_t, std::vector<KvqAttentionParams>> katts; // by d_head
    uint32_t kst_lo = UINT32_MAX, kst_hi = 0, kat_lo = UINT32_MAX, kat_hi = 0, kat_max_q = 0;
    uint32_t rep_max = 0, move_max = 0, att_max = 0, n_rep = 0, n_move = 0, n_att = 0;
    uint32_t lo[3] = {UINT32_MAX, UINT32_MAX, UINT32_MAX}, hi[3] = {0, 0, 0};
    auto track = [&](int k, const PlanItem& it) {
        lo[k] = std::min(lo[k], it.op);
        hi[k] = std::max(hi[k], it.store >= 0 ? std::max(it.op, (uint32_t)it.store) : it.op);
    };
    for (const PlanItem& it : group) {
        const uint32_t i = it.op;
        const zgml_device_op& op = p->ops[i];
        switch (op.kind) {
            case ZGML_DOP_REPEAT:
                if (i < p->hoist_op.size() && p->hoist_op[i]) { // constant: runs once, now (below)
                    hoisted.push_back(make_repeat(p, op.u.repeat));
                    hoisted_max = std::max(hoisted_max, op.u.repeat.n);
                    break;
                }
                reps.push_back(make_repeat(p, op.u.repeat));
                rep_max = std::max(rep_max, op.u.repeat.n);
                n_rep++;
                track(0, it);
                break;
            case ZGML_DOP_SLICE_ASSIGN: {
                MoveParams m{};
                m.kind = 1;
                m.n_elems = op.u.slice_assign.rows * op.u.slice_assign.cols;
                m.sa = make_slice_assign(p, op.u.slice_assign, i);
                moves.push_back(m);
                move_max = std::max(move_max, m.n_elems);
                n_move++;
                track(1, it);
                break;
            }
            case ZGML_DOP_ROPE: {
                MoveParams m{};
                m.kind = 0;
                m.n_elems = op.u.rope.half_d * op.u.rope.seq_len;
                m.rope = make_rope(p, op.u.rope);
                if (it.store >= 0) {
                    const auto& sa = p->ops[it.store].u.slice_assign;
                    m.rope.dst2 = p->bufs[sa.dst];
                    m.rope.dyn_dst2_off = p->dyn_dev + it.store;
                    m.rope.d2_rs = sa.dst_row_stride, m.rope.d2_cs = sa.dst_col_stride;
                    n_move++;
                }
                moves.push_back(m);
                move_max = std::max(move_max, m.n_elems);
                n_move++;
                track(1, it);
                break;
            }
            case ZGML_DOP_ATTENTION: {
                AttentionParams ap = make_attention(p, op.u.attention, i);
                if (it.store >= 0) {
                    const auto& sa = p->ops[it.store].u.slice_assign;
                    ap.dst2 = p->bufs[sa.dst];
                    ap.dyn_dst2_off = p->dyn_dev + it.store;
                    ap.d2_rs = sa.dst_row_stride, ap.d2_cs = sa.dst_col_stride;
                    n_att++;
                    att_store_off.push_back(sa.patch_stride == 0 ? (int64_t)sa.dst_offset : -1); // -1: moves with the position
                } else {
                    att_store_off.push_back(-1);
                }
                atts.push_back(ap);
                att_max = std::max(att_max, op.u.attention.seq_q);
                n_att++;
                track(2, it);
                break;
            }
            case ZGML_DOP_KVQ_STORE: {
                const auto& st = op.u.kvq_store;
                kstores.push_back({p->bufs[st.cache], buf_at(p, st.src, st.src_offset), p->dyn_dev + i, st.d_head, st.block_size, st.n_cols});
                kst_lo = std::min(kst_lo, i), kst_hi = std::max(kst_hi, i);
                break;
            }
            case ZGML_DOP_ATTENTION_KVQ: {
                const auto& a = op.u.attention_kvq;
                KvqAttentionParams kp{};
                kp.dst = buf_at(p, a.dst, a.dst_off), kp.q = buf_at(p, a.q, a.q_off);
                kp.k_cache = p->bufs[a.k], kp.v_cache = p->bufs[a.v];
                kp.mask = a.has_mask ? buf_at(p, a.mask, a.mask_off) : nullptr;
                kp.dyn_seq_kv = p->dyn_dev + i;
                kp.d_head = a.d_head, kp.seq_q = a.seq_q, kp.block_size = a.block_size, kp.n_cols = a.n_cols;
                kp.k_col_start = a.k_col_start, kp.v_col_start = a.v_col_start, kp.q_cs = a.q_cs, kp.dst_cs = a.dst_cs;
                kp.mask_rs = a.mask_rs, kp.mask_cs = a.mask_cs, kp.scale = a.scale;
                katts[a.d_head].push_back(kp);
                kat_lo = std::min(kat_lo, i), kat_hi = std::max(kat_hi, i), kat_max_q = std::max(kat_max_q, a.seq_q);
                break;
            }
            default: {
                Launch L;
                if (make_single(p, i, L)) p->plan.push_back(std::move(L));
            }
        }
    }
    if (!kstores.empty()) {
        const KvqStoreParams* d = upload_params(p, kstores);
        const uint32_t n = (uint32_t)kstores.size();
        p->plan.push_back({ZGML_DOP_KVQ_STORE, n, kst_lo, kst_hi, [=](hipStream_t s) { launch_kvq_store_batch(s, d, n); }});
    }
    for (auto& kv : katts) {
        const KvqAttentionParams* d = upload_params(p, kv.second);
        const uint32_t n = (uint32_t)kv.second.size(), dh = kv.first, mq = kat_max_q;
        AttnSplit sp; // decode launches: long contexts split a head's keys over several workgroups
        if (mq == 1) {
            uint32_t max_kv = 0;
            for (const auto& a : kv.second) max_kv = std::max(max_kv, a.n_cols - std::min(a.n_cols, std::max(a.k_col_start, a.v_col_start)));
            sp = attn_split_for(p, n, dh, max_kv);
        }
        p->plan.push_back({ZGML_DOP_ATTENTION_KVQ, n, kat_lo, kat_hi, [=](hipStream_t s) { launch_kvq_attention_batch(s, d, n, mq, dh, sp); }});
    }
    if (!hoisted.empty()) { // (build_plan runs outside any capture, on the context stream: ordered before the plan's first execution)
        const RepeatParams* d = upload_params(p, hoisted);
        launch_repeat_batch(p->ctx->stream, d, (uint32_t)hoisted.size(), hoisted_max);
    }
    if (!reps.empty()) {
        const RepeatParams* d = upload_params(p, reps);
        const uint32_t n = (uint32_t)reps.size(), mx = rep_max;
        p->plan.push_back({ZGML_DOP_REPEAT, n_rep, lo[0], hi[0], [=](hipStream_t s) { launch_repeat_batch(s, d, n, mx); }});
    }
    if (!moves.empty()) {
        const MoveParams* d = upload_params(p, moves);
        const uint32_t n = (uint32_t)moves.size(), mx = move_max;
        p->plan.push_back({ZGML_DOP_SLICE_ASSIGN, n_move, lo[1], hi[1], [=](hipStream_t s) { launch_move_batch(s, d, n, mx); }});
    }
    if (!atts.empty()) {
        bool dense = true;
        for (const AttentionParams& a : atts) dense = dense && attention_op_dense(a);
        uint32_t rows_dh = dense ? atts[0].d_head : 0; // the streaming kernel: one d_head >= 8 per launch
        for (const AttentionParams& a : atts)
            if (a.d_head != rows_dh || a.d_head < 8) rows_dh = 0;
        const float* zero = p->zero_word;
        const AttentionParams* d = upload_params(p, atts);
        const uint32_t n = (uint32_t)atts.size(), mx = att_max;
        auto sink = std::make_shared<AttnPieceSink>(); // armed by the matmul that reads the heads' row stores, if one follows
        Launch L{ZGML_DOP_ATTENTION, n_att, lo[2], hi[2], [=](hipStream_t s) { launch_attention_batch(s, d, n, mx, dense, rows_dh, zero, *sink); }};
        const AttnRoute route = attention_route(dense, rows_dh, mx, zero); // the kernel launch_attention_batch will pick
        L.tag = attention_route_tag(route);
        // every head stores its rows into one dense [seq_q x cols] matrix (d2_rs == 1, a common row stride) and the tile
        // kernel will run: that matrix may be the next quantized matmul's input
        bool one_matrix = route == AttnRoute::tiles && atts[0].dst2 && atts[0].d2_rs == 1;
        for (const AttentionParams& a : atts)
            one_matrix = one_matrix && a.dst2 == atts[0].dst2 && a.d2_rs == 1 && a.d2_cs == atts[0].d2_cs && a.seq_q == mx;
        std::vector<int64_t> offs = att_store_off;
        std::sort(offs.begin(), offs.end());
        for (size_t h = 0; h < offs.size(); h++) one_matrix = one_matrix && offs[h] == (int64_t)(h * rows_dh); // head h's columns, statically
        if (one_matrix && (uint64_t)rows_dh * n == atts[0].d2_cs) // the heads tile the whole row
            L.hook = std::make_shared<SplitHook>(SplitHook{atts[0].dst2, mx, atts[0].d2_cs, 0, &sink->ap, &sink->S, &sink->cols});
        p->plan.push_back(std::move(L));
    }
}

// ── macro-op fusion around the quantized mat-vecs (M == 1) ───────────────────────────────────
// PROLOGUE  : the elementwise mul (optionally preceded by rmsnorm) that produces a mat-vec's input
//             is computed inside the mat-vec while it stages x (each workgroup recomputes it from
//             L2-resident vectors; workgroup 0 stores the intermediates);
// EPILOGUE  : elementwise / fused_elementwise ops that consume the mat-vec output column-wise are
//             applied by the 16 lanes that own the outputs (residual add, the SiLU chain, ...);
// GROUPING  : mat-vecs of one dependency level that read the same vector (q/k/v, gate/up) share
//             one launch.
// Legality is decided from access spans only (no LLaMA-specific pattern): a macro-op is placed at
// its last member; a member X may be delayed past a non-member C only if X and C do not conflict.
struct Macro {
    std::vector<uint32_t> members; // op indices, ascending
    uint32_t position = 0;         // index of the last member
    bool qmv = false;
    int store = -1;                // rope / attention anchors: the slice_assign folded into them
    uint32_t anchor = 0;           // the qmatmul op (or the rope / attention op)
    QmvPrologue pro;
    uint64_t pro_sig[3] = {0, 0, 0}; // (kind, a, b) identity for grouping
    bool owns_prologue = false;
    uint32_t n_epi = 0;
    QmvEpiStep epi[kMaxEpiSteps];
    OpAccess access;
    // decode attention of one kv group: rope k + K store + V store, and per head rope q +
    // attention (+ row store), all in one launch record per head
    struct Head {
        uint32_t rq, att;
        int row_store;
    };
    std::vector<Head> heads;
    uint32_t rk = 0, sk = 0, sv = 0;
    bool kvq = false; // the same block over quantised caches: sk / sv are kvq_store ops, the heads' `att` attention_kvq ops
    // [add ->] rmsnorm [-> mul] over dense rows (any row count): one launch (RowChainParams)
    bool chain = false;
    int chain_add = -1, chain_mul = -1;
    // elementwise / fused_elementwise ops feeding each other index by index: one launch (EltChainParams)
    bool elt_chain = false;
    EltChainParams elt{};
};

bool ops_conflict(const OpAccess& x, const OpAccess& c) {
    for (const Span& w : x.writes) {
        for (const Span& r : c.reads)
            if (spans_overlap(w, r)) return true;
        for (const Span& w2 : c.writes)
            if (spans_overlap(w, w2)) return true;
    }
    for (const Span& r : x.reads)
        for (const Span& w2 : c.writes)
            if (spans_overlap(r, w2)) return true;
    return false;
}

struct ExactSpan {
    uint16_t buf;
    uint64_t off, n;
    bool operator==(const ExactSpan& o) const { return buf == o.buf && off == o.off && n == o.n; }
    Span span() const { return {buf, off, off + n}; }
};

bool barrier_between(const std::vector<uint64_t>& barriers, uint32_t lo, uint32_t hi) { // a barrier b with lo < b <= hi
    for (uint64_t b : barriers)
        if (b > lo && b <= hi) return true;
    return false;
}

// a declared barrier (zgml_hip_program_set_barriers: a collective of the caller) between launches i and i + 1 keeps them apart
bool barrier_between_launches(const zgml_hip_program* p, size_t i) {
    const Launch &a = p->plan[i], &b = p->plan[i + 1];
    return barrier_between(p->barriers, std::min(a.op_lo, b.op_lo), std::max(a.op_hi, b.op_hi));
}

// a zeroed block of diagnostics stamps in pinned host memory the kernels write through its device mapping (nullptr: none)
unsigned long long* mapped_trace(size_t words) {
    unsigned long long* t = nullptr;
    if (hipHostMalloc((void**)&t, words * sizeof(unsigned long long), hipHostMallocMapped) != hipSuccess) return nullptr;
    memset(t, 0, words * sizeof(unsigned long long));
    return t;
}

void add_access(OpAccess& dst, const OpAccess& src) {
    dst.reads.insert(dst.reads.end(), src.reads.begin(), src.reads.end());
    dst.writes.insert(dst.writes.end(), src.writes.begin(), src.writes.end());
}

bool anchor_ok(zgml_hip_program* p, uint32_t i) {
    const zgml_device_op& op = p->ops[i];
    if (op.kind != ZGML_DOP_QMATMUL || op.u.qmatmul.M != 1) return false;
    const QWeightDev& w = p->qweights[op.u.qmatmul.weight_idx];
    return w.format != QW_RAW && w.format != QW_W8A8 && (op.u.qmatmul.input_offset % 4) == 0; // (W8A8: the reference's arm, launched as it is — no prologue / epilogue fusion)
}

// A grouped q / k / v projection launch directly followed by the decode-attention launch of exactly its heads becomes ONE
// launch (qmatvec.hip: qkv_attn_kernel): the projection's outputs reach the attention as data-tagged
// 8-byte granules (K-on-lanes weights: through per-head-slice counters) instead of through a kernel boundary, and everything the attention can do without them overlaps the
// projection. Only for the shapes that kernel is built for (short K, Q4_0 with f16 scales, d_head 64 / 128, f32 or int8 KV).
void fuse_qkv_attention(zgml_hip_program* p) {
    if (!sw().hip_fuse_qkv_attn || p->ctx->fuse_qkv_off || !p->ctx->handoff_flag_dev) return; // (off for good once a hand-off wait has timed out in this context)
    // Residency: the attention's workgroups spin on granules (or counters) the projection's workgroups of the SAME grid write, and HIP
    // promises neither dispatch order nor co-residency. The launch is only built when the whole grid (1024-thread workgroups)
    // fits the device at ONE workgroup per CU — the occupancy query may say two, but it reads one high near a register-file
    // edge (guide: residency and cooperative launch) and a stranded producer would mean a time-out, not a slowdown; the
    // attention's split count shrinks to fit, and if even one split per head does not fit the two launches stay apart.
    // ZGML_HIP_OPT_FUSE_RESIDENT_WGS overrides the capacity (0 refuses every fusion).
    const uint64_t resident_cap = p->ctx->opt_fuse_resident_wgs >= 0 ? (uint64_t)p->ctx->opt_fuse_resident_wgs : (uint64_t)std::max(p->ctx->n_cu, 1);
    for (size_t i = 0; i + 1 < p->plan.size(); i++) {
        const auto qd = p->plan[i].qmv_desc;
        const auto ad = p->plan[i + 1].adec_desc;
        if (!qd || !ad) continue;
        const QmvLaunch& L = *qd;
        if (barrier_between_launches(p, i)) continue;
        const bool kon = L.parts[0].w.format == QW_Q4K && L.K > 2048; // the 256-thread form of the launch (qkv_attn_kon_kernel)
        if (L.n_parts != 3 || (L.K > 2048 && !(kon && sw().hip_fuse_qkv_attn_kon)) || L.pro.kind == QMV_PRO_NONE || (ad->dh != 64 && ad->dh != 128) || L.trace) continue;
        if (kon && L.pro.kind != QMV_PRO_PRENORM) continue; // (an in-kernel rmsnorm prologue runs eight waves: launch_packed_kon)
        const bool kvq = ad->kvq;
        bool ok = true;
        for (uint32_t t = 0; t < 3; t++) ok = ok && L.parts[t].n_epi == 0 && (L.parts[t].w.format == QW_Q4 || L.parts[t].w.format == QW_Q4K) && L.parts[t].w.scale_f16;
        const uint32_t nh = ad->nh, dh = ad->dh;
        ok = ok && (uint64_t)nh * dh == L.parts[0].w.N && L.parts[1].w.N == L.parts[2].w.N && L.parts[1].w.N % dh == 0;
        const uint32_t n_kv = ok ? (uint32_t)(L.parts[1].w.N / dh) : 0;
        ok = ok && n_kv != 0 && nh % n_kv == 0;
        std::vector<uint32_t> idx(3 * (size_t)nh); // (counter form: each record's q / k / v counter)
        std::vector<char> head_seen(nh, 0);
        bool group_order = true; // record r is a head of kv group r / (nh / n_kv): the block map's assumption (qkv_colocate.h)
        for (uint32_t r = 0; ok && r < nh; r++) { // the records are not in head order: each one's head from its pointers
            const AttnDecodeParams& a = ad->host[r];
            const ptrdiff_t qo = a.q_src - L.parts[0].dst, ko = a.k_src - L.parts[1].dst, vo = a.v_src - L.parts[2].dst;
            ok = qo >= 0 && qo % dh == 0 && (uint64_t)qo < (uint64_t)nh * dh && ko >= 0 && ko % dh == 0 && (uint64_t)ko < (uint64_t)n_kv * dh && vo == ko &&
                 a.kvq_block == (kvq ? 32u : 0u);
            if (!ok) break;
            const uint32_t h = (uint32_t)(qo / dh), kvh = (uint32_t)(ko / dh);
            ok = !head_seen[h] && kvh == h / (nh / n_kv);
            head_seen[h] = 1; // (granule form: the kernel finds the record's granules from the same pointer differences, DecodeHandoff)
            group_order = group_order && kvh == r / (nh / n_kv);
            idx[3 * r] = h, idx[3 * r + 1] = nh + kvh, idx[3 * r + 2] = nh + n_kv + kvh;
        }
        if (!ok) continue;
        uint32_t n_sp = ad->sp.splits ? ad->sp.splits : 1;
        uint64_t n_mv = 0;
        for (uint32_t t = 0; t < 3; t++) n_mv += L.parts[t].w.N / 16;
        uint64_t cap = resident_cap;
        if (kon && p->ctx->opt_fuse_resident_wgs < 0) {
            // 256-thread workgroups: what the occupancy query admits (four per CU at 127 registers: 1024; the 7B launch is 768 projection
            // workgroups + 32 heads x up to 8 splits = 1024). No margin here, unlike the 1024-thread form: with 4 instead of 8 splits
            // the launch LOSES at long contexts (position 1900: 590 against 632 tok/s unfused; with 8: 644), and the projection's
            // workgroups have the lower ids — should fewer be resident than the query says, the attention's workgroups queue behind
            // them instead of spinning beside them (no overlap then, nothing worse); a stranded wait is still bounded and loud.
            const int per_cu = qkv_attn_kon_blocks_per_cu(ad->dh, kvq);
            cap = per_cu > 0 ? (uint64_t)per_cu * (uint64_t)std::max(p->ctx->n_cu, 1) * (uint64_t)sw().hip_fuse_kon_cap_eighths / 8 : 0;
        }
        if (n_mv + nh > cap) continue; // not even one attention workgroup per head beside the projection's: two launches
        // (the 256-thread form only with ALL the splits the stand-alone attention would use: with fewer it loses at long contexts —
        // 7B dimensions with 4 of 8: 590 against 632 tok/s at position 1900 — so a wider model keeps its two launches)
        if (kon && p->ctx->opt_fuse_resident_wgs < 0 && (cap - n_mv) / nh < n_sp) continue;
        n_sp = (uint32_t)std::min<uint64_t>(n_sp, (cap - n_mv) / nh);
        for (uint32_t t = 0; kon && t < 3; t++) ok = ok && L.parts[t].w.format == QW_Q4K;
        if (!ok) continue;
        if (kon && p->ctx->opt_fuse_resident_wgs < 0) {
            // ... and the grid it comes to is CENSUSED once per context and size: the kernel's own census instantiation counts its
            // workgroups and each waits (bounded) for all of them — co-residency measured, not inferred
            const uint32_t grid = (uint32_t)(n_mv + (uint64_t)nh * n_sp);
            const uint64_t key = ((uint64_t)ad->dh << 40) | ((uint64_t)(kvq ? 1 : 0) << 32) | grid;
            auto it = p->ctx->census.find(key);
            if (it == p->ctx->census.end()) {
                const int r = sw().hip_fuse_census ? qkv_attn_kon_census(p->ctx->stream, ad->dh, kvq, grid) : -1;
                it = p->ctx->census.emplace(key, r).first;
                if (r == 0) fprintf(stderr, "[zgml_hip] the fused q/k/v + attention launch of %u workgroups is NOT co-resident on this device (census): two launches instead\n", grid);
            }
            if (it->second == 0) continue;
        }
        // (The O projection — the single-matrix launch that reads exactly the heads' row stores — does NOT ride along. Measured: 93
        // launches per SmolLM-135M token instead of 123, parity green, and SLOWER — 1714-1734 against 1772 tok/s: that edge is
        // all-to-all (every column group of the projection needs every head), its hand-off costs more than the boundary it replaces.)
        // the launch's hand-off block, zeroed ONCE (its state runs on across executions and graph replays). Granule form (handoff_gen.h):
        // [(nh + 2 n_kv) * dh granules of 8 bytes: a column group's 16 are one 128-byte line (hipMalloc aligns to 256)]
        // [one generation word per projection column group] [one per attention workgroup]
        // Counter form (the K-on-lanes launch: CounterHandoff): [one counter per 128 bytes] [3 `seen` words per attention workgroup] [idx]
        const size_t n_gran = ((size_t)nh + 2 * n_kv) * dh, n_cnt = 32 * ((size_t)nh + 2 * n_kv);
        const size_t bytes = kon ? (n_cnt + (size_t)nh * n_sp * 3 + 1 + idx.size()) * 4 : (n_gran * 8 + (n_mv + (size_t)nh * n_sp) * 4 + 15) / 16 * 16;
        void* block = nullptr;
        if (hipMalloc(&block, bytes) != hipSuccess) continue;
        if (memset_sync(p->ctx->stream, block, 0, bytes) != hipSuccess) {
            hipFree(block);
            continue;
        }
        p->fuse_owned.push_back(block); // (freed by the next build_plan, after its stream sync)
        uint32_t* const timeout = p->ctx->handoff_flag_dev;
        QkvHandoffBlock hb;
        if (kon) {
            hb.counters = (uint32_t*)block, hb.seen = hb.counters + n_cnt;
            uint32_t* const idx_dev = hb.seen + (size_t)nh * n_sp * 3 + 1;
            if (h2d_sync(p->ctx->stream, idx_dev, idx.data(), idx.size() * 4) != hipSuccess) continue;
            hb.idx = idx_dev;
        } else {
            hb.granules = (unsigned long long*)block;
            hb.producer_gen = (uint32_t*)(hb.granules + n_gran), hb.consumer_gen = hb.producer_gen + n_mv;
            hb.group_order = group_order;
            const size_t n_wg = (size_t)n_mv + (size_t)nh * n_sp;
            if (sw().hip_attn_trace && (hb.xcc_trace = (uint32_t*)mapped_trace((n_wg + 1) / 2))) // (diagnostics build: where every workgroup of the launch ran)
                p->xcc_traces.push_back({hb.xcc_trace, (uint32_t)n_mv, nh, n_kv, dh, n_sp});
        }
        const AttnDecodeParams* d = ad->dev;
        AttnSplit sp = ad->sp;
        sp.splits = n_sp; // (possibly fewer than the stand-alone launch would use: the residency guard above)
        const uint32_t n_ops = p->plan[i].n_ops + p->plan[i + 1].n_ops, lo = std::min(p->plan[i].op_lo, p->plan[i + 1].op_lo),
                       hi = std::max(p->plan[i].op_hi, p->plan[i + 1].op_hi);
        Launch F{ZGML_DOP_QMATMUL, n_ops, lo, hi, [=](hipStream_t s) {
                     if (!launch_qkv_attention(s, L, d, nh, n_kv, dh, sp, hb, timeout, kvq)) {
                         launch_qmatvec_fused(s, L);
                         launch_attention_decode_batch(s, d, nh, dh, sp, kvq);
                     }
                 }};
        p->plan[i] = std::move(F);
        p->plan.erase(p->plan.begin() + (ptrdiff_t)i + 1);
    }
}

// The decoder layer of a short-K model as launches that end at a K-split (ksplit.hip): in the plan built above a
// layer is [q/k/v (rmsnorm prologue)] [decode attention] [O (+ residual)] [gate / up (rmsnorm prologue, SiLU chain)] [down (product
// prologue, + residual)]. Here
//   [q/k/v] [attention] [O]   ->  [ks_proj] [ks_attn_o]   (each head's workgroup adds its partial of the O projection)
//   [gate / up] [down]        ->  [ks_mlp]                (each 32-column workgroup adds its partial of the down projection)
// and the O / down projections' outputs and residual sums become DEFERRED vectors (kernels.h: KsVec): the next launch of the plan
// sums the partials in its prologue and its workgroup 0 stores the absorbed ops' buffers. When that next launch is not one that can
// (anything but a ks_proj / ks_mlp / the final rmsnorm -> mul row chain reading exactly that vector), a one-workgroup launch
// materialises the vector at once. Conditions are checked on spans and pointers, not on a model name: n-on-lanes Q4_0 weights with
// f16 scales (ks_weight_ok), K <= 2048, d_head 64 / 128, residual and norm outputs that do not alias their inputs.
void fuse_ksplit(zgml_hip_program* p) {
    p->has_deferred = false;
    if (!p->ksplit || p->ksplit_off || !p->barriers.empty()) return;
    auto overlap = [](const float* a, size_t na, const float* b, size_t nb) { return a && b && a < b + nb && b < a + na; };
    auto residual_epi = [](const QmvPart& pt) {
        return pt.n_epi == 1 && pt.epi[0].op == ZGML_OP_ADD && pt.epi[0].operand && pt.epi[0].operand != pt.dst && pt.epi[0].store && pt.epi[0].store != pt.dst;
    };
    // outputs the consumer's workgroup 0 stores late must not overlap anything the other workgroups still read
    auto norm_in_safe = [&](const KsNormIn& in) {
        const size_t K = in.K;
        const float* outs[4] = {in.x.sum_dst, in.x.add_dst, in.store_mid, in.store_x};
        for (const float* o : outs) {
            if (!o) continue;
            if (overlap(o, K, in.x.base, K) || overlap(o, K, in.gamma, K) || overlap(o, K, in.x.parts, K * in.x.n_parts)) return false;
            for (const float* o2 : outs)
                if (o2 && o2 != o && overlap(o, K, o2, K)) return false;
        }
        return true;
    };
    std::vector<Launch> out;
    KsVec pend{};
    uint32_t pend_K = 0;
    bool have_pend = false;
    uint32_t pend_lo = 0, pend_hi = 0;
    auto flush = [&]() { // nobody took the deferred vector: materialise it now
        if (!have_pend) return;
        KsNormIn in;
        in.x = pend, in.K = pend_K;
        Launch M{ZGML_DOP_ELEMENTWISE, 0, pend_lo, pend_hi, [in](hipStream_t s) { launch_ks_norm(s, in); }};
        M.tag = "ks-materialise";
        out.push_back(std::move(M));
        have_pend = false;
    };
    float *parts_o = nullptr, *parts_d = nullptr; // one block each for the whole program: producer and consumer follow each other in stream order
    size_t parts_o_n = 0, parts_d_n = 0;
    auto grow_parts = [&](float*& blk, size_t& have, size_t want) -> bool {
        if (have >= want) return true;
        float* nb = nullptr;
        if (hipMalloc((void**)&nb, want * sizeof(float)) != hipSuccess || memset_sync(p->ctx->stream, nb, 0, want * sizeof(float)) != hipSuccess) {
            if (nb) hipFree(nb);
            return false;
        }
        p->fuse_owned.push_back(nb); // (an earlier, smaller block stays owned too: launches already emitted point into it)
        blk = nb, have = want;
        return true;
    };
    std::vector<Launch>& plan = p->plan;
    size_t i = 0;
    uint32_t n_fused = 0;
    auto new_trace = [&](const char* what) -> unsigned long long* { // diagnostics build + ZGML_HIP_KS_TRACE=1
        unsigned long long* t = nullptr;
        if (!sw().hip_ks_trace || p->ks_traces.size() >= 24 || !(t = mapped_trace(32))) return nullptr;
        p->ks_traces.push_back({t, what});
        return t;
    };
    while (i < plan.size()) {
        // ---- [q/k/v] [attention] [O]
        if (i + 2 < plan.size() && plan[i].qmv_desc && plan[i + 1].adec_desc && plan[i + 2].qmv_desc) {
            const QmvLaunch &Q = *plan[i].qmv_desc, &O = *plan[i + 2].qmv_desc;
            const AdecDesc& A = *plan[i + 1].adec_desc;
            bool ok = Q.n_parts == 3 && Q.pro.kind == QMV_PRO_RMSNORM_MUL && !Q.trace && !O.trace && O.n_parts == 1 && O.pro.kind == QMV_PRO_NONE && residual_epi(O.parts[0]) &&
                      !O.next.xg_out && (A.dh == 64 || A.dh == 128) && O.K == A.nh * A.dh && ks_weight_ok(O.parts[0].w);
            for (uint32_t t = 0; ok && t < 3; t++) ok = Q.parts[t].n_epi == 0 && ks_weight_ok(Q.parts[t].w);
            std::vector<char> seen_head(A.nh, 0);
            uint8_t head_of[64] = {0};
            ok = ok && A.nh <= 64;
            for (uint32_t r = 0; ok && r < A.nh; r++) { // every head row-stores into the O projection's input at h * d_head, every h once
                const AttnDecodeParams& a = A.host[r];
                ok = a.att.dst2 == O.pro.a && a.att.d2_rs == 1 && a.att.dyn_dst2_off >= p->dyn_dev && a.att.dyn_dst2_off < p->dyn_dev + p->ops.size() && a.att.dst_rs == 1 &&
                     ((uintptr_t)a.att.dst2 % 16) == 0;
                if (!ok) break;
                const zgml_device_op& so = p->ops[(size_t)(a.att.dyn_dst2_off - p->dyn_dev)];
                ok = so.kind == ZGML_DOP_SLICE_ASSIGN && so.u.slice_assign.patch_stride == 0 && so.u.slice_assign.dst_offset % A.dh == 0 &&
                     so.u.slice_assign.dst_offset / A.dh < A.nh && !seen_head[so.u.slice_assign.dst_offset / A.dh];
                if (ok) seen_head[so.u.slice_assign.dst_offset / A.dh] = 1, head_of[r] = (uint8_t)(so.u.slice_assign.dst_offset / A.dh);
            }
            KsProjLaunch PL;
            KsAttnOLaunch AL;
            if (ok) {
                PL.in.K = Q.K, PL.in.gamma = Q.pro.b, PL.in.eps = Q.pro.eps, PL.in.store_mid = Q.pro.store_mid, PL.in.store_x = Q.pro.store_x;
                if (have_pend && pend.add_dst == Q.pro.a && pend_K == Q.K)
                    PL.in.x = pend;
                else
                    PL.in.x.base = Q.pro.a;
                PL.n_parts = 3;
                for (uint32_t t = 0; t < 3; t++) PL.w[t] = Q.parts[t].w, PL.dst[t] = Q.parts[t].dst;
                const size_t N = O.parts[0].w.N;
                ok = ks_proj_ok(PL) && norm_in_safe(PL.in) && grow_parts(parts_o, parts_o_n, (size_t)A.nh * N);
                PL.trace = new_trace("ks-proj"), AL.trace = new_trace("ks-attn-o");
                memcpy(AL.head_of, head_of, sizeof head_of);
                AL.dev = A.dev, AL.n_heads = A.nh, AL.d_head = A.dh, AL.sp = A.sp, AL.kvq = A.kvq, AL.wo = O.parts[0].w, AL.parts_out = parts_o;
                ok = ok && ks_attn_o_ok(AL);
            }
            if (ok) {
                const bool took = PL.in.x.n_parts != 0;
                if (!took) flush();
                have_pend = false;
                // ... as ONE launch when the whole grid is resident (the attention's workgroups spin on the projection's: one 768-thread
                // workgroup per CU is what is counted on; the split count shrinks to fit) and the context's hand-offs have not timed out
                bool fused = false;
                if (sw().hip_ksplit_fuse_a && !p->ctx->fuse_qkv_off && p->ctx->handoff_flag_dev && ks_layer_a_ok(PL, AL)) {
                    const uint32_t nh = A.nh, dh = A.dh;
                    const uint32_t n_kv = (uint32_t)(Q.parts[1].w.N / dh);
                    std::vector<uint32_t> idx(3 * (size_t)nh);
                    bool hk = n_kv != 0 && Q.parts[1].w.N % dh == 0 && Q.parts[2].w.N == Q.parts[1].w.N && (uint64_t)nh * dh == Q.parts[0].w.N && nh % n_kv == 0;
                    for (uint32_t r = 0; hk && r < nh; r++) { // each record's q / k / v counters from its pointers into the projections' outputs
                        const AttnDecodeParams& ar = A.host[r];
                        const ptrdiff_t qo = ar.q_src - Q.parts[0].dst, ko = ar.k_src - Q.parts[1].dst, vo = ar.v_src - Q.parts[2].dst;
                        hk = qo >= 0 && qo % dh == 0 && (uint64_t)qo < (uint64_t)nh * dh && ko >= 0 && ko % dh == 0 && (uint64_t)ko < (uint64_t)n_kv * dh && vo == ko;
                        if (hk) idx[3 * r] = (uint32_t)(qo / dh), idx[3 * r + 1] = nh + (uint32_t)(ko / dh), idx[3 * r + 2] = nh + n_kv + (uint32_t)(ko / dh);
                    }
                    const uint64_t cap = p->ctx->opt_fuse_resident_wgs >= 0 ? (uint64_t)p->ctx->opt_fuse_resident_wgs : (uint64_t)std::max(p->ctx->n_cu, 1);
                    const uint32_t n_pw = ks_layer_a_proj_wgs(PL);
                    uint32_t n_sp = AL.sp.splits ? AL.sp.splits : 1;
                    if (hk && n_pw + nh <= cap) {
                        n_sp = (uint32_t)std::min<uint64_t>(n_sp, (cap - n_pw) / nh);
                        const size_t n_cnt = 32 * ((size_t)nh + 2 * n_kv), words = n_cnt + (size_t)nh * n_sp * 3 + 3 * (size_t)nh;
                        uint32_t* block = nullptr;
                        if (hipMalloc((void**)&block, words * 4) == hipSuccess) {
                            p->fuse_owned.push_back(block);
                            uint32_t *counters = block, *seen = block + n_cnt, *idx_dev = seen + (size_t)nh * n_sp * 3;
                            if (memset_sync(p->ctx->stream, block, 0, words * 4) == hipSuccess && h2d_sync(p->ctx->stream, idx_dev, idx.data(), idx.size() * 4) == hipSuccess) {
                                KsAttnOLaunch AF = AL;
                                AF.sp.splits = n_sp;
                                uint32_t* const timeout = p->ctx->handoff_flag_dev;
                                Launch LA{ZGML_DOP_QMATMUL, plan[i].n_ops + plan[i + 1].n_ops + plan[i + 2].n_ops, std::min({plan[i].op_lo, plan[i + 1].op_lo, plan[i + 2].op_lo}),
                                          std::max({plan[i].op_hi, plan[i + 1].op_hi, plan[i + 2].op_hi}), [PL, AF, AL, n_kv, counters, idx_dev, seen, timeout](hipStream_t s) {
                                              if (!launch_ks_layer_a(s, PL, AF, n_kv, counters, idx_dev, seen, timeout)) {
                                                  launch_ks_proj(s, PL);
                                                  launch_ks_attn_o(s, AL);
                                              }
                                          }};
                                LA.tag = took ? "ks-layer-a (sums the deferred vector): q / k / v + attention + partial O projection"
                                              : "ks-layer-a: q / k / v + attention + partial O projection";
                                out.push_back(std::move(LA));
                                fused = true;
                            }
                        }
                    }
                }
                if (!fused) {
                    Launch L1{ZGML_DOP_QMATMUL, plan[i].n_ops, plan[i].op_lo, plan[i].op_hi, [PL](hipStream_t s) { launch_ks_proj(s, PL); }};
                    L1.tag = took ? "ks-proj (sums the deferred vector)" : "ks-proj";
                    Launch L2{ZGML_DOP_ATTENTION, plan[i + 1].n_ops + plan[i + 2].n_ops, std::min(plan[i + 1].op_lo, plan[i + 2].op_lo), std::max(plan[i + 1].op_hi, plan[i + 2].op_hi),
                              [AL](hipStream_t s) { launch_ks_attn_o(s, AL); }};
                    L2.tag = "ks-attention + partial O projection";
                    out.push_back(std::move(L1));
                    out.push_back(std::move(L2));
                }
                pend = KsVec{O.parts[0].epi[0].operand, parts_o, A.nh, O.parts[0].dst, O.parts[0].epi[0].store};
                pend_K = (uint32_t)O.parts[0].w.N, have_pend = true, pend_lo = plan[i + 2].op_lo, pend_hi = plan[i + 2].op_hi;
                i += 3, n_fused++;
                continue;
            }
        }
        // ---- [gate / up] [down]
        if (i + 1 < plan.size() && plan[i].qmv_desc && plan[i + 1].qmv_desc) {
            const QmvLaunch &G = *plan[i].qmv_desc, &D = *plan[i + 1].qmv_desc;
            const QmvPart &ga = G.parts[0], &up = G.parts[1];
            const QmvEpiStep* st = ga.epi;
            bool ok = G.n_parts == 2 && G.pro.kind == QMV_PRO_RMSNORM_MUL && !G.pair_out && !G.trace && !D.trace && D.n_parts == 1 && D.pro.kind == QMV_PRO_MUL && D.pro.store_x &&
                      residual_epi(D.parts[0]) && !D.next.xg_out;
            // the SiLU chain exactly as build_qmv_args recognises it (NEG, EXP [store], ADD vector, RECIP, MUL by the gate [store])
            ok = ok && ga.n_epi == 5 && st[0].op == ZGML_OP_NEG && !st[0].store && st[1].op == ZGML_OP_EXP && st[1].store && st[2].op == ZGML_OP_ADD && st[2].operand &&
                 st[2].operand != ga.dst && st[2].operand != st[1].store && !st[2].store && st[3].op == ZGML_OP_RECIP && !st[3].store && st[4].op == ZGML_OP_MUL &&
                 st[4].operand == ga.dst && st[4].store && up.n_epi == 0;
            ok = ok && ((D.pro.a == st[4].store && D.pro.b == up.dst) || (D.pro.b == st[4].store && D.pro.a == up.dst)) && D.K == ga.w.N;
            KsMlpLaunch ML;
            if (ok) {
                ML.in.K = G.K, ML.in.gamma = G.pro.b, ML.in.eps = G.pro.eps, ML.in.store_mid = G.pro.store_mid, ML.in.store_x = G.pro.store_x;
                if (have_pend && pend.add_dst == G.pro.a && pend_K == G.K)
                    ML.in.x = pend;
                else
                    ML.in.x.base = G.pro.a;
                ML.gate = ga.w, ML.up = up.w, ML.down = D.parts[0].w;
                ML.gate_out = ga.dst, ML.up_out = up.dst, ML.exp_out = st[1].store, ML.silu_out = st[4].store, ML.prod_out = D.pro.store_x, ML.ones = st[2].operand;
                ok = grow_parts(parts_d, parts_d_n, (size_t)ks_mlp_parts(ML) * ML.down.N);
                ML.parts_out = parts_d, ML.trace = new_trace("ks-mlp");
                ok = ok && ks_mlp_ok(ML) && norm_in_safe(ML.in);
            }
            if (ok) {
                const bool took = ML.in.x.n_parts != 0;
                if (!took) flush();
                have_pend = false;
                Launch L{ZGML_DOP_QMATMUL, plan[i].n_ops + plan[i + 1].n_ops, std::min(plan[i].op_lo, plan[i + 1].op_lo), std::max(plan[i].op_hi, plan[i + 1].op_hi),
                         [ML](hipStream_t s) { launch_ks_mlp(s, ML); }};
                L.tag = took ? "ks-mlp (sums the deferred vector): gate / up + partial down projection" : "ks-mlp: gate / up + partial down projection";
                out.push_back(std::move(L));
                pend = KsVec{D.parts[0].epi[0].operand, parts_d, ks_mlp_parts(ML), D.parts[0].dst, D.parts[0].epi[0].store};
                pend_K = (uint32_t)ML.down.N, have_pend = true, pend_lo = plan[i + 1].op_lo, pend_hi = plan[i + 1].op_hi;
                i += 2, n_fused++;
                continue;
            }
        }
        // ---- the deferred vector's rmsnorm -> mul row chain (the final norm in front of the LM head): one workgroup does both
        if (have_pend && plan[i].rc_desc && plan[i].rc_rows == 1) {
            const RowChainParams& rc = *plan[i].rc_desc;
            KsNormIn in;
            in.x = pend, in.K = pend_K, in.gamma = rc.mul_other, in.eps = rc.eps, in.store_mid = rc.norm_dst, in.store_x = rc.mul_dst;
            if (!rc.a0 && !rc.ap && rc.src == pend.add_dst && rc.mul_other && rc.mul_dst && rc.cols == pend_K && ks_norm_ok(in) && norm_in_safe(in)) {
                Launch L{ZGML_DOP_RMSNORM, plan[i].n_ops, std::min(plan[i].op_lo, pend_lo), std::max(plan[i].op_hi, pend_hi), [in](hipStream_t s) { launch_ks_norm(s, in); }};
                L.tag = "ks-norm (sums the deferred vector): rmsnorm -> mul";
                out.push_back(std::move(L));
                have_pend = false;
                i++;
                continue;
            }
        }
        flush();
        out.push_back(std::move(plan[i]));
        i++;
    }
    flush();
    if (n_fused) {
        plan = std::move(out);
        p->has_deferred = true;
    }
}

// A mat-vec launch with a residual-add epilogue (h = y + r: the O / down projections) that is DIRECTLY followed by the launch
// whose rmsnorm -> mul(gamma) prologue consumes h prepares that prologue (kernels.h: QmvNextNorm / QMV_PRO_PRENORM): it also
// stores h * gamma and, per 16 columns, the sum of h^2. The consumer then streams one vector instead of two — x (16 KB at
// K = 4096) stays in a CU's L1 across the workgroups it hosts, x and gamma together do not (tools/exp/kon.hip: +0.5 us at
// 4096^2, +0.8 at 4096 x 11008, +1.8 at 4096 x 32000) — and needs no sum over x. Consumers: K-on-lanes launches (QW_Q4K) and, since
// round 4, the x-direct n-on-lanes launches of short-K models (qmv_prenorm_ok: SmolLM-135M's q/k/v and gate/up, whose in-kernel
// prologue — second vector, sum of squares, barrier — cost 1.1 us of a 2.6 us launch by the stamps).
void arm_prenorm(zgml_hip_program* p) {
    if (!sw().hip_prenorm) return;
    for (size_t i = 1; i < p->plan.size(); i++) {
        const auto C = p->plan[i].qmv_desc, P = p->plan[i - 1].qmv_desc;
        if (!C || !P || C->pro.kind != QMV_PRO_RMSNORM_MUL) continue;
        bool ok = true;
        uint64_t cols = 0;
        for (uint32_t t = 0; t < C->n_parts; t++) cols += C->parts[t].w.N;
        for (uint32_t t = 0; t < C->n_parts; t++) ok = ok && C->parts[t].w.format == C->parts[0].w.format && qmv_prenorm_ok(C->parts[t].w, C->K, cols, 1);
        const QmvPart& pp = P->parts[0];
        ok = ok && P->n_parts == 1 && pp.w.format != QW_RAW && pp.w.N == C->K && pp.n_epi == 1 && pp.epi[0].op == ZGML_OP_ADD && pp.epi[0].operand &&
             pp.epi[0].operand != pp.dst && pp.epi[0].store == C->pro.a && C->K % 16 == 0 && !P->next.xg_out;
        if (!ok) continue;
        if (barrier_between_launches(p, i - 1)) continue;
        const size_t need = ((size_t)C->K + C->K / 16) * sizeof(float);
        if (p->prenorm_bytes < need) { // one block for the whole program: the pairs follow each other in stream order
            float* blk = nullptr;
            if (hipMalloc((void**)&blk, need) != hipSuccess || memset_sync(p->ctx->stream, blk, 0, need) != hipSuccess) {
                if (blk) hipFree(blk);
                continue;
            }
            p->owned.push_back(blk);
            p->prenorm_buf = blk, p->prenorm_bytes = need;
        }
        float *xg = p->prenorm_buf, *ssq = p->prenorm_buf + C->K;
        P->next = QmvNextNorm{C->pro.b, xg, ssq};
        C->pro.kind = QMV_PRO_PRENORM;
        C->pro.xg = xg, C->pro.ssq = ssq, C->pro.n_ssq = C->K / 16;
    }
}

// gate / up -> down: the grouped launch {gate with the SiLU chain, up} directly followed by the mat-vec whose MUL prologue
// multiplies exactly silu(gate) and up becomes a PAIR launch (qmatvec.hip: qmatvec_kon_pair_kernel): one workgroup computes
// the same 16 columns of both matrices (x is loaded once) and stores the product itself; the down projection then streams
// one vector with no prologue (x = a * b per lane meant two 44 KB vectors per workgroup at Llama-2-7B's d_ff). K-on-lanes
// weights, and since round 4 the x-direct n-on-lanes launches of short-K models (qmv_pair_ok: SmolLM-135M, whose down projection
// spent 0.5 us more than the O projection in front of its first load on the second vector).
void arm_pair(zgml_hip_program* p) {
    // (ZGML_QMV_EPI_SILU=0 asks for the SiLU chain through the generic step interpreter: the pair launch IS a fused SiLU epilogue)
    if (!sw().hip_pair || !sw().qmv_epi_silu) return;
    for (size_t i = 1; i < p->plan.size(); i++) {
        const auto D = p->plan[i].qmv_desc, G = p->plan[i - 1].qmv_desc;
        if (!D || !G || D->pro.kind != QMV_PRO_MUL || !D->pro.store_x || G->n_parts != 2 || G->pair_out) continue;
        const QmvPart &ga = G->parts[0], &up = G->parts[1];
        const QmvEpiStep* st = ga.epi;
        // the SiLU chain exactly as build_qmv_args recognises it (NEG, EXP [store], ADD vector, RECIP, MUL by the gate [store])
        bool ok = ga.n_epi == 5 && st[0].op == ZGML_OP_NEG && !st[0].store && st[1].op == ZGML_OP_EXP && st[1].store && st[2].op == ZGML_OP_ADD &&
                  st[2].operand && st[2].operand != ga.dst && st[2].operand != st[1].store && !st[2].store && st[3].op == ZGML_OP_RECIP && !st[3].store &&
                  st[4].op == ZGML_OP_MUL && st[4].operand == ga.dst && st[4].store && up.n_epi == 0;
        ok = ok && ga.w.format == up.w.format && qmv_pair_ok(ga.w) && qmv_pair_ok(up.w) && ga.w.N == up.w.N && ga.w.K == up.w.K && (ga.w.N / 16) % 2 == 0 && ga.w.N == D->K &&
             (G->pro.kind == QMV_PRO_NONE || G->pro.kind == QMV_PRO_PRENORM) && D->n_parts == 1;
        // the product's operands: silu(gate) and up, in either order (an f32 product does not depend on it)
        ok = ok && ((D->pro.a == st[4].store && D->pro.b == up.dst) || (D->pro.b == st[4].store && D->pro.a == up.dst));
        // (n-on-lanes form under a prepared norm: every workgroup stores a 16-element slice of the absorbed ops' outputs, and a pair
        // launch has one workgroup per column group of ONE matrix: it needs N >= K of them)
        ok = ok && (ga.w.format == QW_Q4K || G->pro.kind != QMV_PRO_PRENORM || ga.w.N >= G->K);
        // the two weights back to back in the arenas (the pair kernel finds part 1 from part 0)
        ok = ok && (const char*)up.w.qs == (const char*)ga.w.qs + ga.w.qs_bytes && (const char*)up.w.sc == (const char*)ga.w.sc + ga.w.sc_bytes;
        ok = ok && ((uintptr_t)G->pro.a % 16 == 0) && (G->K % 4 == 0) && (G->pro.kind != QMV_PRO_PRENORM || (uintptr_t)G->pro.xg % 16 == 0);
        if (!ok) continue;
        if (barrier_between_launches(p, i - 1)) continue;
        G->pair_out = D->pro.store_x;
        QmvPrologue plain;
        plain.a = D->pro.store_x;
        D->pro = plain;
    }
}

// What the fusion passes of build_fused_plan share: the ops, their access spans (the schedule's) and which ops are taken — by a
// prologue (`owner`) or by a macro-op (`in_macro`). Every pass claims greedily in program order, and the passes run in a fixed
// order: which op a macro-op absorbs depends on everything claimed before it.
struct Planner {
    zgml_hip_program* p;
    const std::vector<zgml_device_op>& ops;
    const std::vector<OpAccess>& access; // per op
    const size_t n;
    std::vector<int> owner;     // op -> -2 while a prologue holds it, else -1
    std::vector<char> in_macro; // op -> absorbed by a macro-op
    std::vector<Macro> macros;
    // prologues: one absorbed producer chain per input vector, shared by all its consumers
    struct ProInfo {
        QmvPrologue pro;
        std::vector<uint32_t> absorbed;  // P (and Q)
        std::vector<uint32_t> consumers; // qmatmul ops
        OpAccess reads;                  // what a non-owner consumer reads instead of P.dst
    };
    std::vector<ProInfo> pros;
    std::vector<int> pro_of; // qmatmul op -> its prologue in `pros`, else -1

    explicit Planner(zgml_hip_program* p)
        : p(p), ops(p->ops), access(p->sched.access), n(p->ops.size()), owner(n, -1), in_macro(n, 0), pro_of(n, -1) {}

    // latest op < before writing into q
    int last_writer(const Span& q, uint32_t before) const {
        for (int j = (int)before - 1; j >= 0; j--)
            for (const Span& w : access[j].writes)
                if (spans_overlap(w, q)) return j;
        return -1;
    }
    // the ops after `after` that read q, up to the first one that overwrites it
    std::vector<uint32_t> readers_until_overwrite(const Span& q, uint32_t after) const {
        std::vector<uint32_t> out;
        for (uint32_t j = after + 1; j < n; j++) {
            for (const Span& r : access[j].reads)
                if (spans_overlap(r, q)) {
                    out.push_back(j);
                    break;
                }
            for (const Span& w : access[j].writes)
                if (spans_overlap(w, q)) return out;
        }
        return out;
    }
    // members may be delayed to `last` only if they conflict with no non-member in between
    bool delay_legal(const std::vector<uint32_t>& members, uint32_t last) const {
        for (uint32_t x : members)
            for (uint32_t c = x + 1; c < last; c++) {
                if (std::find(members.begin(), members.end(), c) != members.end()) continue;
                if (ops_conflict(access[x], access[c])) return false;
            }
        return !members.empty() && !barrier_between(p->barriers, members.front(), last);
    }
    // ... and among themselves: inside one launch a member's store races with whatever another member reads or writes at ANOTHER
    // index (delay_legal sees only the non-members, a pass's pattern checks only the chain value). `exempt(x, w, y, s, s_write)`:
    // the overlap of x's store w with y's span s is one the pass threads through — at the same index by the same lanes, or in
    // registers. Anything else refuses the fusion.
    template <typename Exempt>
    bool members_disjoint(const std::vector<uint32_t>& members, Exempt exempt) const {
        for (uint32_t x : members)
            for (const Span& w : access[x].writes)
                for (uint32_t y : members) {
                    if (y == x) continue;
                    for (const Span& s : access[y].reads)
                        if (spans_overlap(w, s) && !exempt(x, w, y, s, false)) return false;
                    for (const Span& s : access[y].writes)
                        if (spans_overlap(w, s) && !exempt(x, w, y, s, true)) return false;
                }
        return true;
    }
    static bool same_span(const Span& a, const Span& b) { // the same elements (runs as wide as their period are dense)
        auto dense = [](const Span& x) { return x.period == 0 || x.width == x.period; };
        return a.buf == b.buf && a.lo == b.lo && a.hi == b.hi &&
               ((dense(a) && dense(b)) || (a.period == b.period && a.width == b.width));
    }
    bool free_op(int j) const { return j >= 0 && !in_macro[j] && owner[j] == -1; }

    bool exact_dst(uint32_t i, ExactSpan& out) const { // contiguous vector outputs only
        const zgml_device_op& o = ops[i];
        switch (o.kind) {
            case ZGML_DOP_ELEMENTWISE: out = {o.u.elementwise.dst, o.u.elementwise.dst_offset, o.u.elementwise.n}; return true;
            case ZGML_DOP_FUSED_ELEMENTWISE:
                out = {o.u.fused_elementwise.dst, o.u.fused_elementwise.dst_offset, o.u.fused_elementwise.n};
                return true;
            case ZGML_DOP_RMSNORM:
                if (o.u.rmsnorm.rows != 1) return false;
                out = {o.u.rmsnorm.dst, o.u.rmsnorm.dst_offset, o.u.rmsnorm.cols};
                return true;
            case ZGML_DOP_QMATMUL:
                if (o.u.qmatmul.M != 1) return false;
                out = {o.u.qmatmul.dst, o.u.qmatmul.dst_offset, o.u.qmatmul.N};
                return true;
            default: return false;
        }
    }

    // ---- constant repeats (see zgml_hip_program::hoist_op)
    void hoist_constant_repeats() {
        p->hoist_op.assign(n, 0);
        p->hoist_guard.assign(p->bufs.size(), 0);
        if (!sw().hip_hoist_repeat || !p->hoist_ok || !p->barriers.empty()) return;
        std::vector<uint32_t> writers(p->bufs.size(), 0);
        for (size_t i = 0; i < n; i++) {
            std::vector<uint16_t> seen;
            for (const Span& w : access[i].writes)
                if (w.buf < writers.size() && std::find(seen.begin(), seen.end(), w.buf) == seen.end()) writers[w.buf]++, seen.push_back(w.buf);
        }
        for (size_t i = 0; i < n; i++) {
            if (ops[i].kind != ZGML_DOP_REPEAT) continue;
            const auto& r = ops[i].u.repeat;
            if (r.src >= writers.size() || r.dst >= writers.size() || r.src == r.dst || writers[r.src] != 0 || writers[r.dst] != 1) continue;
            p->hoist_op[i] = 1;
            p->hoist_guard[r.src] = p->hoist_guard[r.dst] = 1;
        }
    }

    // ---- prologues: the elementwise mul (optionally preceded by rmsnorm) that produces a mat-vec's input
    void prologues() {
        for (uint32_t i = 0; i < n; i++) {
            if (!anchor_ok(p, i) || pro_of[i] >= 0) continue;
            const auto& q = ops[i].u.qmatmul;
            const ExactSpan in{q.input, q.input_offset, q.K};
            const int P = last_writer(in.span(), i);
            if (P < 0 || owner[P] >= 0) continue;
            const zgml_device_op& po = ops[P];
            if (po.kind != ZGML_DOP_ELEMENTWISE || po.u.elementwise.op != ZGML_OP_MUL) continue;
            const auto& e = po.u.elementwise;
            if (!(ExactSpan{e.dst, e.dst_offset, e.n} == in)) continue;
            if ((e.dst_offset % 4) || (e.src0_offset % 4) || (e.src1_offset % 4)) continue;
            const std::vector<uint32_t> readers = readers_until_overwrite(in.span(), (uint32_t)P);
            bool ok = !readers.empty();
            for (uint32_t r : readers) {
                if (!anchor_ok(p, r)) ok = false;
                else {
                    const auto& rq = ops[r].u.qmatmul;
                    if (!(ExactSpan{rq.input, rq.input_offset, rq.K} == in)) ok = false;
                    if (rq.K > qmv_max_prologue_k(p->qweights[rq.weight_idx])) ok = false;
                }
            }
            if (!ok) continue;
            ProInfo info;
            info.absorbed = {(uint32_t)P};
            info.consumers = readers;
            info.pro.kind = QMV_PRO_MUL;
            info.pro.a = buf_at(p, e.src0, e.src0_offset);
            info.pro.b = buf_at(p, e.src1, e.src1_offset);
            info.pro.store_x = buf_at(p, e.dst, e.dst_offset);
            info.reads.reads = access[P].reads;
            const ProInfo mul_only = info;
            // rmsnorm feeding one side of the mul?
            for (int side = 0; side < 2; side++) {
                const ExactSpan sp = side == 0 ? ExactSpan{e.src0, e.src0_offset, e.n} : ExactSpan{e.src1, e.src1_offset, e.n};
                const int Q = last_writer(sp.span(), (uint32_t)P);
                if (Q < 0 || owner[Q] >= 0 || ops[Q].kind != ZGML_DOP_RMSNORM) continue;
                const auto& rn = ops[Q].u.rmsnorm;
                ExactSpan qd{};
                if (!exact_dst((uint32_t)Q, qd) || !(qd == sp) || (rn.src_offset % 4) || (rn.dst_offset % 4)) continue;
                const std::vector<uint32_t> qreaders = readers_until_overwrite(sp.span(), (uint32_t)Q);
                if (qreaders.size() != 1 || qreaders[0] != (uint32_t)P) continue;
                info.absorbed = {(uint32_t)Q, (uint32_t)P};
                info.pro.kind = QMV_PRO_RMSNORM_MUL;
                info.pro.eps = rn.eps;
                info.pro.a = buf_at(p, rn.src, rn.src_offset);
                info.pro.b = side == 0 ? buf_at(p, e.src1, e.src1_offset) : buf_at(p, e.src0, e.src0_offset);
                info.pro.store_mid = buf_at(p, rn.dst, rn.dst_offset);
                info.reads.reads = access[Q].reads;
                info.reads.reads.push_back(side == 0 ? access[P].reads[1] : access[P].reads[0]);
                break;
            }
            // the absorbed ops are delayed to the first consumer, and their inputs must survive until the last. A rmsnorm form
            // that fails falls back to the plain mul form (mul_only) before the prologue is given up.
            auto legal = [&](const ProInfo& info) {
                if (!delay_legal(info.absorbed, info.consumers.front())) return false;
                // every consumer recomputes the prologue from its inputs, so each input must keep its value
                // from the op that originally read it (Q for the rmsnorm source, P for the rest) up to the
                // last consumer
                bool inputs_live = true;
                auto live = [&](const Span& r, uint32_t from) {
                    for (uint32_t c = from + 1; c < info.consumers.back() && inputs_live; c++) {
                        if (std::find(info.absorbed.begin(), info.absorbed.end(), c) != info.absorbed.end()) continue;
                        for (const Span& w : access[c].writes)
                            if (spans_overlap(r, w)) inputs_live = false;
                    }
                };
                if (info.pro.kind == QMV_PRO_RMSNORM_MUL) {
                    live(info.reads.reads[0], info.absorbed.front()); // x, read by the rmsnorm
                    live(info.reads.reads[1], (uint32_t)P);            // gamma (repeat output), read by the mul
                } else {
                    for (const Span& r : info.reads.reads) live(r, (uint32_t)P);
                }
                if (!inputs_live || barrier_between(p->barriers, info.absorbed.front(), info.consumers.back())) return false;
                // in the launch every workgroup reads the prologue's inputs while workgroup 0 stores the absorbed ops' outputs: no
                // store may meet an input (a gain over the norm's output, x = x * g) or the other store
                for (uint32_t x : info.absorbed)
                    for (const Span& w : access[x].writes) {
                        for (const Span& r : info.reads.reads)
                            if (spans_overlap(w, r)) return false;
                        for (uint32_t y : info.absorbed)
                            for (const Span& w2 : access[y].writes)
                                if (y != x && spans_overlap(w, w2)) return false;
                    }
                return true;
            };
            if (!legal(info)) {
                if (info.pro.kind != QMV_PRO_RMSNORM_MUL || !legal(mul_only)) continue;
                info = mul_only;
            }
            const int id = (int)pros.size();
            for (uint32_t c : info.consumers) pro_of[c] = id;
            for (uint32_t x : info.absorbed) owner[x] = -2; // claimed; macro id assigned below
            pros.push_back(std::move(info));
        }
    }

    // the mat-vec macro without its prologue: the anchor reads its input vector as it is, the epilogue stays
    void drop_prologue(Macro& m) {
        const auto& q = ops[m.anchor].u.qmatmul;
        std::vector<uint32_t> keep;
        for (uint32_t x : m.members)
            if (x >= m.anchor) keep.push_back(x);
            else in_macro[x] = 0;
        m.members = keep;
        m.pro = QmvPrologue{};
        m.pro.a = buf_at(p, q.input, q.input_offset);
        m.pro_sig[0] = 0, m.pro_sig[1] = (uint64_t)(uintptr_t)m.pro.a, m.pro_sig[2] = 0;
        m.access = OpAccess{};
        for (uint32_t x : m.members) add_access(m.access, access[x]);
    }

    // ---- one macro per mat-vec anchor: (prologue) + anchor + epilogue chain
    void matvec_macros() {
        for (uint32_t i = 0; i < n; i++) {
            if (!anchor_ok(p, i)) continue;
            Macro m;
            m.qmv = true;
            m.anchor = i;
            const auto& q = ops[i].u.qmatmul;
            m.pro.kind = QMV_PRO_NONE;
            m.pro.a = buf_at(p, q.input, q.input_offset);
            OpAccess acc = access[i];
            if (pro_of[i] >= 0) {
                const ProInfo& info = pros[pro_of[i]];
                m.pro = info.pro;
                m.owns_prologue = info.consumers.front() == i;
                if (m.owns_prologue) {
                    for (uint32_t x : info.absorbed) {
                        m.members.push_back(x);
                        add_access(acc, access[x]);
                    }
                } else { // recompute without storing: read the prologue's inputs instead of its output
                    m.pro.store_mid = nullptr;
                    m.pro.store_x = nullptr;
                    acc.reads = info.reads.reads;
                }
            }
            m.pro_sig[0] = m.pro.kind, m.pro_sig[1] = (uint64_t)(uintptr_t)m.pro.a, m.pro_sig[2] = (uint64_t)(uintptr_t)m.pro.b;
            m.members.push_back(i);
            // in the launch every workgroup reads the whole input vector (and the prologue's inputs), workgroup 0 stores the
            // prologue's outputs (prologues() keeps those apart), and the lanes that own a column run the epilogue on it: an
            // overlap is legal only as the prologue's output = the anchor's input, or as one span of the anchor's output /
            // the epilogue met again at the same columns
            auto exempt = [&](uint32_t x, const Span& w, uint32_t y, const Span& s, bool s_write) {
                if (x < i && y < i) return true;
                if (x < i && y == i && !s_write) return same_span(w, s);
                if (x < i || y < i || (y == i && !s_write)) return false;
                return same_span(w, s);
            };
            // a consumer that recomputes a prologue it does not own reads the prologue's inputs in every workgroup
            auto shared_inputs_kept = [&](const std::vector<uint32_t>& mem) {
                if (pro_of[i] < 0 || m.owns_prologue) return true;
                for (uint32_t x : mem)
                    for (const Span& w : access[x].writes)
                        for (const Span& r : pros[pro_of[i]].reads.reads)
                            if (spans_overlap(w, r)) return false;
                return true;
            };
            // epilogue chain
            ExactSpan cur{q.dst, q.dst_offset, q.N};
            uint32_t cur_idx = i;
            for (;;) {
                int B = -1;
                for (uint32_t r : readers_until_overwrite(cur.span(), cur_idx))
                    if (!in_macro[r] && owner[r] == -1 &&
                        (ops[r].kind == ZGML_DOP_ELEMENTWISE || ops[r].kind == ZGML_DOP_FUSED_ELEMENTWISE)) {
                        B = (int)r;
                        break;
                    }
                if (B < 0) break;
                const zgml_device_op& bo = ops[B];
                QmvEpiStep steps[kMaxEpiSteps];
                uint32_t ns = 0;
                ExactSpan bdst{};
                bool ok = exact_dst((uint32_t)B, bdst) && bdst.n == cur.n;
                if (ok && bo.kind == ZGML_DOP_ELEMENTWISE) {
                    const auto& e = bo.u.elementwise;
                    const bool binary = e.op == ZGML_OP_ADD || e.op == ZGML_OP_MUL;
                    const ExactSpan s0sp{e.src0, e.src0_offset, e.n}, s1sp{e.src1, e.src1_offset, e.n};
                    if (s0sp == cur)
                        steps[ns++] = {e.op, 0, binary ? buf_at(p, e.src1, e.src1_offset) : nullptr, nullptr};
                    else if (binary && s1sp == cur)
                        steps[ns++] = {e.op, 1, buf_at(p, e.src0, e.src0_offset), nullptr};
                    else
                        ok = false;
                } else if (ok) {
                    const auto& f = bo.u.fused_elementwise;
                    ok = ExactSpan{f.src, f.src_offset, f.n} == cur && f.n_steps <= (uint32_t)kMaxEpiSteps;
                    for (uint32_t t = 0; ok && t < f.n_steps; t++) {
                        const bool binary = f.steps[t].op == ZGML_OP_ADD || f.steps[t].op == ZGML_OP_MUL;
                        steps[ns++] = {f.steps[t].op, f.steps[t].is_swapped,
                                       binary ? buf_at(p, f.steps[t].secondary_buf, f.steps[t].secondary_offset) : nullptr, nullptr};
                    }
                }
                if (!ok || ns == 0 || m.n_epi + ns > (uint32_t)kMaxEpiSteps) break;
                std::vector<uint32_t> trial = m.members;
                trial.push_back((uint32_t)B);
                if (!delay_legal(trial, (uint32_t)B) || !members_disjoint(trial, exempt) || !shared_inputs_kept(trial)) break;
                steps[ns - 1].store = buf_at(p, bdst.buf, bdst.off);
                for (uint32_t t = 0; t < ns; t++) m.epi[m.n_epi++] = steps[t];
                m.members.push_back((uint32_t)B);
                in_macro[B] = 1;
                add_access(acc, access[B]);
                cur = bdst;
                cur_idx = (uint32_t)B;
            }
            if ((m.members.size() > 1 && (!delay_legal(m.members, m.members.back()) || !members_disjoint(m.members, exempt))) ||
                !shared_inputs_kept(m.members)) { // absorbed prologue + epilogue together
                // fall back to the bare anchor (keeps correctness trivially)
                for (uint32_t x : m.members)
                    if (x != i) in_macro[x] = 0;
                m.members = {i}, m.n_epi = 0, m.owns_prologue = false;
                drop_prologue(m);
                if (pro_of[i] >= 0) { // the prologue ops must then run on their own
                    for (uint32_t x : pros[pro_of[i]].absorbed) owner[x] = -1;
                    for (uint32_t c : pros[pro_of[i]].consumers) pro_of[c] = -1;
                }
            } else {
                m.access = acc;
            }
            std::sort(m.members.begin(), m.members.end());
            m.position = m.members.back();
            for (uint32_t x : m.members) in_macro[x] = 1;
            macros.push_back(std::move(m));
        }
        // consumers whose prologue was revoked after their macro was built: rebuild plainly
        for (Macro& m : macros)
            if (m.qmv && m.pro.kind != QMV_PRO_NONE && pro_of[m.anchor] < 0) drop_prologue(m);
    }

    // ---- decode attention (seq_q == 1): per kv group {rope k, K store, V store} + per head {rope q, attention, row store}
    // become one launch record per head (AttnDecodeParams). The new K/V column is recomputed by every head of the group from
    // the projections and never re-read from the cache, so the heads of a group need no ordering among themselves.
    // kvq: the same fold over quantised KV caches (extension ops kvq_store / attention_kvq). The fused kernel quantises the new
    // column exactly as storeColumn does and uses the quantised values, so cache bytes and outputs equal the op-by-op plan's.
    void decode_attention(bool kvq) {
        if (!sw().hip_attn_decode || (kvq && !sw().hip_attn_decode_kvq)) return;
        auto aligned4 = [&](uint16_t buf, uint64_t off) { return ((uintptr_t)buf_at(p, buf, off) % 16) == 0; };
        auto rope_ok = [&](int r, uint16_t dst, uint64_t dst_off, uint32_t dh) { // one column of d_head values written to (dst, dst_off)
            if (r < 0 || in_macro[r] || ops[r].kind != ZGML_DOP_ROPE) return false;
            const auto& ro = ops[r].u.rope;
            return ro.dst == dst && ro.dst_off == dst_off && 2 * ro.half_d == dh && ro.seq_len == 1 && ro.src_rs == 1 && aligned4(ro.src, ro.src_off) &&
                   aligned4(ro.cos_sin, ro.cs_off) && aligned4(ro.dst, ro.dst_off);
        };
        struct Cand {
            uint32_t rq, att, rk, sk, sv;
            int row_store;
        };
        std::map<uint32_t, std::vector<Cand>> groups; // by K store op
        for (uint32_t i = 0; i < n; i++) {
            if (in_macro[i] || ops[i].kind != (kvq ? ZGML_DOP_ATTENTION_KVQ : ZGML_DOP_ATTENTION)) continue;
            // per form: the attention's own checks and its K / V stores; then the query, the key rope and the head's output
            uint16_t q, dst, k_src;
            uint64_t q_off, dst_off, k_src_off;
            uint32_t dh, dst_cs;
            int sk, sv;
            if (!kvq) {
                const auto& t = ops[i].u.attention;
                dh = t.d_head;
                if (t.seq_q != 1 || (dh & (dh - 1)) || dh < 8 || dh > 256 || t.q_rs != 1 || t.k_rs != 1 || t.v_rs != 1 || t.dst_rs != 1 ||
                    t.k_cs % 4 || t.v_cs % 4 || t.seq_kv == 0 || !aligned4(t.q, t.q_off) || !aligned4(t.k, t.k_off) ||
                    !aligned4(t.v, t.v_off) || !aligned4(t.dst, t.dst_off))
                    continue;
                // the slabs must hold seq_kv (compile-time bound) whole columns: speculative reads stay inside
                const uint64_t k_end = t.k_off + (uint64_t)(t.seq_kv - 1) * t.k_cs + dh, v_end = t.v_off + (uint64_t)(t.seq_kv - 1) * t.v_cs + dh;
                if (k_end > p->sizes[t.k] || v_end > p->sizes[t.v]) continue;
                // K / V stores of the dynamic column
                sk = last_writer(Span{t.k, t.k_off, k_end}, i), sv = last_writer(Span{t.v, t.v_off, v_end}, i);
                if (sk < 0 || sv < 0 || in_macro[sk] || in_macro[sv] || ops[sk].kind != ZGML_DOP_SLICE_ASSIGN || ops[sv].kind != ZGML_DOP_SLICE_ASSIGN) continue;
                const auto &ks = ops[sk].u.slice_assign, &vs = ops[sv].u.slice_assign;
                if (ks.dst != t.k || !ks.patch_stride || ks.patch_stride != t.k_cs || ks.dst_base_offset != t.k_off || ks.rows != dh ||
                    ks.cols != 1 || ks.dst_row_stride != 1 || ks.src_row_stride != 1)
                    continue;
                if (vs.dst != t.v || !vs.patch_stride || vs.patch_stride != t.v_cs || vs.dst_base_offset != t.v_off || vs.rows != dh ||
                    vs.cols != 1 || vs.dst_row_stride != 1 || vs.src_row_stride != 1 || !aligned4(vs.src, vs.src_offset))
                    continue;
                q = t.q, q_off = t.q_off, dst = t.dst, dst_off = t.dst_off, dst_cs = t.dst_cs, k_src = ks.src, k_src_off = ks.src_offset;
            } else {
                const auto& t = ops[i].u.attention_kvq;
                dh = t.d_head;
                if (t.seq_q != 1 || t.block_size != 32 || (dh != 32 && dh != 64 && dh != 128 && dh != 256) || t.k_col_start || t.v_col_start ||
                    t.seq_kv == 0 || t.n_cols == 0 || !aligned4(t.q, t.q_off) || !aligned4(t.dst, t.dst_off) || t.k == t.v)
                    continue;
                const uint64_t cache_elems = (uint64_t)t.n_cols * dh / 4 + (uint64_t)t.n_cols * (dh / 32);
                if (cache_elems > p->sizes[t.k] || cache_elems > p->sizes[t.v]) continue;
                // (the key loop addresses cache rows, scales and mask words as a uniform base + a 32-bit byte offset: attention_decode.h)
                if (cache_elems * 4 >= (1ull << 32) || (t.has_mask && (uint64_t)t.n_cols * t.mask_rs * 4 >= (1ull << 32))) continue;
                // K / V stores: the last writers anywhere into the caches
                sk = last_writer(Span{t.k, 0, p->sizes[t.k]}, i), sv = last_writer(Span{t.v, 0, p->sizes[t.v]}, i);
                if (sk < 0 || sv < 0 || in_macro[sk] || in_macro[sv] || ops[sk].kind != ZGML_DOP_KVQ_STORE || ops[sv].kind != ZGML_DOP_KVQ_STORE) continue;
                const auto &ks = ops[sk].u.kvq_store, &vs = ops[sv].u.kvq_store;
                if (ks.cache != t.k || vs.cache != t.v || ks.d_head != dh || vs.d_head != dh || ks.block_size != 32 || vs.block_size != 32 ||
                    ks.n_cols != t.n_cols || vs.n_cols != t.n_cols || !aligned4(vs.src, vs.src_offset))
                    continue;
                q = t.q, q_off = t.q_off, dst = t.dst, dst_off = t.dst_off, dst_cs = t.dst_cs, k_src = ks.src, k_src_off = ks.src_offset;
            }
            // query rope, and the key rope that feeds the K store
            const int rq = last_writer(Span{q, q_off, q_off + dh}, i);
            if (!rope_ok(rq, q, q_off, dh)) continue;
            const int rk = last_writer(Span{k_src, k_src_off, k_src_off + dh}, (uint32_t)sk);
            if (!rope_ok(rk, k_src, k_src_off, dh)) continue;
            // optional row store of the dense head output
            int row_store = -1;
            if (dst_cs == dh) {
                for (uint32_t r : readers_until_overwrite(Span{dst, dst_off, dst_off + dh}, i)) {
                    if (in_macro[r] || ops[r].kind != ZGML_DOP_SLICE_ASSIGN) continue;
                    const auto& sa = ops[r].u.slice_assign;
                    if (sa.src != dst || sa.src_offset != dst_off || sa.rows != dh || sa.cols != 1 || sa.src_row_stride != 1) continue;
                    row_store = (int)r;
                    break;
                }
            }
            groups[(uint32_t)sk].push_back({(uint32_t)rq, i, (uint32_t)rk, (uint32_t)sk, (uint32_t)sv, row_store});
        }
        for (auto& kv : groups) {
            const std::vector<Cand>& hs = kv.second;
            bool same = true;
            for (const Cand& c : hs) same = same && c.rk == hs[0].rk && c.sv == hs[0].sv;
            if (!same) continue;
            Macro m;
            m.kvq = kvq;
            m.rk = hs[0].rk, m.sk = hs[0].sk, m.sv = hs[0].sv;
            m.members = {m.rk, m.sk, m.sv};
            for (const Cand& c : hs) {
                m.members.push_back(c.rq);
                m.members.push_back(c.att);
                if (c.row_store >= 0) m.members.push_back((uint32_t)c.row_store);
                m.heads.push_back({c.rq, c.att, c.row_store});
            }
            std::sort(m.members.begin(), m.members.end());
            if (std::adjacent_find(m.members.begin(), m.members.end()) != m.members.end()) continue; // an op claimed twice
            m.position = m.members.back();
            if (!delay_legal(m.members, m.position)) continue;
            // one record per head recomputes the new K / V column from the projections (rope k -> K store -> every head's
            // attention, V store -> every head's attention) and runs rope q -> attention -> row store: only those edges may meet
            auto role = [&](uint32_t o) -> int { // 0 rk, 1 sk, 2 sv, 3 + 3h rq, 4 + 3h att, 5 + 3h row store of head h
                if (o == m.rk) return 0;
                if (o == m.sk) return 1;
                if (o == m.sv) return 2;
                for (size_t h = 0; h < m.heads.size(); h++) {
                    if (o == m.heads[h].rq) return 3 + 3 * (int)h;
                    if (o == m.heads[h].att) return 4 + 3 * (int)h;
                    if ((int)o == m.heads[h].row_store) return 5 + 3 * (int)h;
                }
                return -1;
            };
            auto exempt = [&](uint32_t x, const Span&, uint32_t y, const Span&, bool s_write) {
                if (s_write) return false;
                const int rx = role(x), ry = role(y);
                if (rx == 0) return ry == 1;
                if (rx == 1 || rx == 2) return ry >= 4 && (ry - 4) % 3 == 0;
                return rx >= 3 && (rx - 3) % 3 != 2 && ry == rx + 1;
            };
            if (!members_disjoint(m.members, exempt)) continue;
            for (uint32_t x : m.members) {
                add_access(m.access, access[x]);
                in_macro[x] = 1;
            }
            m.anchor = hs[0].att;
            macros.push_back(std::move(m));
        }
    }

    // ---- rope -> slice_assign (K into the cache) and attention -> slice_assign (head output into the concatenated buffer):
    // the copy of the anchor's dense output is done by the anchor itself
    void store_folds() {
        for (uint32_t i = 0; i < n; i++) {
            if (in_macro[i] || (ops[i].kind != ZGML_DOP_ROPE && ops[i].kind != ZGML_DOP_ATTENTION)) continue;
            ExactSpan out{};
            uint32_t rows, cols, srs, scs;
            if (ops[i].kind == ZGML_DOP_ROPE) {
                const auto& r = ops[i].u.rope;
                rows = 2 * r.half_d, cols = r.seq_len, srs = 1, scs = rows;
                out = {r.dst, r.dst_off, (uint64_t)rows * cols};
            } else {
                const auto& t = ops[i].u.attention;
                rows = t.d_head, cols = t.seq_q, srs = t.dst_rs, scs = t.dst_cs;
                if (srs != 1 || scs != rows) continue; // dense head output only
                out = {t.dst, t.dst_off, (uint64_t)rows * cols};
            }
            for (uint32_t r : readers_until_overwrite(out.span(), i)) {
                if (in_macro[r] || ops[r].kind != ZGML_DOP_SLICE_ASSIGN) continue;
                const auto& sa = ops[r].u.slice_assign;
                if (sa.src != out.buf || sa.src_offset != out.off || sa.rows != rows || sa.cols != cols ||
                    sa.src_row_stride != srs || sa.src_col_stride != scs)
                    continue;
                // the anchor stores each element twice (its output, the slice): the slice may meet the anchor's spans only as
                // the copied output itself
                if (!delay_legal({i, r}, r) || !members_disjoint({i, r}, [&](uint32_t x, const Span& w, uint32_t y, const Span& s, bool s_write) {
                        return x == i && y == r && !s_write && same_span(w, s);
                    }))
                    continue;
                Macro m;
                m.members = {i, r};
                m.position = r;
                m.anchor = i;
                m.store = (int)r;
                m.access = access[i];
                add_access(m.access, access[r]);
                in_macro[i] = in_macro[r] = 1;
                macros.push_back(std::move(m));
                break;
            }
        }
    }

    // ---- [elementwise add ->] rmsnorm [-> elementwise mul] on the same dense rows: one launch instead of three
    // (the M > 1 / prefill form of what the mat-vec prologue does at M = 1; every intermediate is still stored)
    void row_chains() {
        const bool enabled = sw().hip_row_chain;
        for (uint32_t i = 0; enabled && i < n; i++) {
            if (!free_op((int)i) || ops[i].kind != ZGML_DOP_RMSNORM) continue;
            const auto& rn = ops[i].u.rmsnorm;
            const uint64_t cnt = (uint64_t)rn.rows * rn.cols;
            if (!cnt) continue;
            const ExactSpan S{rn.src, rn.src_offset, cnt}, D{rn.dst, rn.dst_offset, cnt};
            int A = last_writer(S.span(), i), P = -1;
            if (free_op(A) && ops[A].kind == ZGML_DOP_ELEMENTWISE && ops[A].u.elementwise.op == ZGML_OP_ADD) {
                const auto& e = ops[A].u.elementwise;
                if (!(ExactSpan{e.dst, e.dst_offset, e.n} == S)) A = -1;
            } else {
                A = -1;
            }
            const std::vector<uint32_t> readers = readers_until_overwrite(D.span(), i);
            if (readers.size() == 1 && free_op((int)readers[0]) && ops[readers[0]].kind == ZGML_DOP_ELEMENTWISE &&
                ops[readers[0]].u.elementwise.op == ZGML_OP_MUL) {
                const auto& e = ops[readers[0]].u.elementwise;
                const bool s0 = ExactSpan{e.src0, e.src0_offset, e.n} == D, s1 = ExactSpan{e.src1, e.src1_offset, e.n} == D;
                if (e.n == cnt && (s0 != s1)) P = (int)readers[0];
            }
            // widest legal chain first
            const std::vector<std::vector<int>> tries = {{A, (int)i, P}, {(int)i, P}, {A, (int)i}};
            for (const auto& t : tries) {
                std::vector<uint32_t> mem;
                for (int x : t)
                    if (x >= 0) mem.push_back((uint32_t)x);
                if (mem.size() < 2 || std::find(t.begin(), t.end(), -1) != t.end()) continue;
                if (!delay_legal(mem, mem.back())) continue;
                // the launch reads every input row up front and recomputes the chain values (launch_row_chain keeps ONE workgroup
                // per row when a store meets a read): members may meet only on the same elements, and a member reads what an
                // earlier one stored only as the chain value itself (the add's sum as the norm's source, the norm as the mul's side)
                const int add = t.front() == (int)i ? -1 : t.front(), mul = t.back() == (int)i ? -1 : t.back();
                auto exempt = [&](uint32_t x, const Span& w, uint32_t y, const Span& s, bool s_write) {
                    if (!same_span(w, s)) return false;
                    if (s_write || y < x) return true;
                    return ((int)x == add && y == i) || (x == i && (int)y == mul);
                };
                if (!members_disjoint(mem, exempt)) continue;
                Macro m;
                m.chain = true;
                m.members = mem;
                m.position = mem.back();
                m.anchor = i;
                m.chain_add = t.front() == (int)i ? -1 : t.front();
                m.chain_mul = t.back() == (int)i ? -1 : t.back();
                for (uint32_t x : mem) {
                    add_access(m.access, access[x]);
                    in_macro[x] = 1;
                }
                macros.push_back(std::move(m));
                break;
            }
        }
    }

    // ---- elementwise chains (the SiLU chain and its product with the up projection at M > 1, ...): ops over the same n
    // elements where each consumes its predecessor's output at the same index become one launch
    void elementwise_chains() {
        const bool enabled = sw().hip_elt_chain;
        auto is_elt = [&](uint32_t j) { return ops[j].kind == ZGML_DOP_ELEMENTWISE || ops[j].kind == ZGML_DOP_FUSED_ELEMENTWISE; };
        // append op j's steps; `cur` = the chain value's span (nullptr for the first op, which sets src)
        auto append = [&](EltChainParams& c, uint32_t j, const ExactSpan* cur, ExactSpan& out) -> bool {
            const zgml_device_op& o = ops[j];
            if (o.kind == ZGML_DOP_ELEMENTWISE) {
                const auto& e = o.u.elementwise;
                const bool binary = e.op == ZGML_OP_ADD || e.op == ZGML_OP_MUL;
                const ExactSpan a{e.src0, e.src0_offset, e.n}, b{e.src1, e.src1_offset, e.n};
                if (c.n_steps + 1 > (uint32_t)kMaxChainSteps) return false;
                ChainStepDev st{e.op, 0, nullptr, buf_at(p, e.dst, e.dst_offset)};
                if (!cur) {
                    c.src = buf_at(p, e.src0, e.src0_offset), c.n = e.n;
                    st.secondary = binary ? buf_at(p, e.src1, e.src1_offset) : nullptr;
                } else if (a == *cur && !(binary && b == *cur)) {
                    st.secondary = binary ? buf_at(p, e.src1, e.src1_offset) : nullptr;
                } else if (binary && b == *cur && !(a == *cur)) {
                    st.swapped = 1, st.secondary = buf_at(p, e.src0, e.src0_offset);
                } else {
                    return false;
                }
                c.steps[c.n_steps++] = st;
                out = {e.dst, e.dst_offset, e.n};
                return true;
            }
            const auto& f = o.u.fused_elementwise;
            if (f.n_steps == 0 || c.n_steps + f.n_steps > (uint32_t)kMaxChainSteps) return false;
            if (!cur)
                c.src = buf_at(p, f.src, f.src_offset), c.n = f.n;
            else if (!(ExactSpan{f.src, f.src_offset, f.n} == *cur))
                return false;
            for (uint32_t t = 0; t < f.n_steps; t++) {
                const bool binary = f.steps[t].op == ZGML_OP_ADD || f.steps[t].op == ZGML_OP_MUL;
                c.steps[c.n_steps++] = {f.steps[t].op, f.steps[t].is_swapped,
                                        binary ? buf_at(p, f.steps[t].secondary_buf, f.steps[t].secondary_offset) : nullptr, nullptr};
            }
            c.steps[c.n_steps - 1].store = buf_at(p, f.dst, f.dst_offset);
            out = {f.dst, f.dst_offset, f.n};
            return true;
        };
        for (uint32_t i = 0; enabled && i < n; i++) {
            if (!free_op((int)i) || !is_elt(i)) continue;
            Macro m;
            ExactSpan cur{};
            if (!append(m.elt, i, nullptr, cur)) continue;
            m.members = {i};
            for (;;) {
                bool grown = false;
                for (uint32_t r : readers_until_overwrite(cur.span(), m.members.back())) {
                    if (!free_op((int)r) || !is_elt(r) || std::find(m.members.begin(), m.members.end(), r) != m.members.end()) continue;
                    EltChainParams trial_p = m.elt;
                    ExactSpan nxt{};
                    if (!append(trial_p, r, &cur, nxt) || nxt.n != cur.n) continue;
                    std::vector<uint32_t> trial = m.members;
                    trial.push_back(r);
                    // thread i runs every step at index i (an operand an earlier step stored keeps the step-by-step reads:
                    // launch_eltwise_chain): members may meet only on the same elements
                    if (!delay_legal(trial, r) || !members_disjoint(trial, [](uint32_t, const Span& w, uint32_t, const Span& s, bool) { return same_span(w, s); }))
                        continue;
                    m.elt = trial_p, m.members = trial, cur = nxt, grown = true;
                    break;
                }
                if (!grown) break;
            }
            if (m.members.size() < 2) continue;
            m.elt_chain = true;
            m.position = m.members.back();
            m.anchor = i;
            for (uint32_t x : m.members) {
                add_access(m.access, access[x]);
                in_macro[x] = 1;
            }
            macros.push_back(std::move(m));
        }
    }

    // ---- everything else is a singleton
    void singletons() {
        for (uint32_t i = 0; i < n; i++) {
            if (in_macro[i]) continue;
            Macro m;
            m.members = {i};
            m.position = i;
            m.access = access[i];
            macros.push_back(std::move(m));
        }
    }

    // the per-head records of a decode-attention macro, appended to their launch's group (by d_head; int8-KV heads apart)
    void decode_records(const Macro& m, std::map<uint32_t, std::vector<AttnDecodeParams>>& by_dh) {
        const auto& kr = ops[m.rk].u.rope;
        bool first_head = true;
        for (const Macro::Head& h : m.heads) {
            const auto& qr = ops[h.rq].u.rope;
            AttnDecodeParams a{};
            if (m.kvq) {
                const auto& t = ops[h.att].u.attention_kvq;
                const auto &ks = ops[m.sk].u.kvq_store, &vs = ops[m.sv].u.kvq_store;
                a.att.dst = buf_at(p, t.dst, t.dst_off), a.att.q = a.q_rot = buf_at(p, t.q, t.q_off);
                a.att.mask = t.has_mask ? buf_at(p, t.mask, t.mask_off) : p->zero_word;
                a.att.mask_rs = t.has_mask ? t.mask_rs : 0, a.att.mask_cs = t.has_mask ? t.mask_cs : 0;
                a.att.d_head = t.d_head, a.att.seq_q = 1, a.att.dyn_seq_kv = p->dyn_dev + h.att, a.att.scale = t.scale;
                a.att.q_rs = 1, a.att.q_cs = t.q_cs, a.att.dst_rs = 1, a.att.dst_cs = t.dst_cs;
                a.k_cache = p->bufs[ks.cache], a.v_cache = p->bufs[vs.cache];
                a.v_src = buf_at(p, vs.src, vs.src_offset);
                a.max_kv = t.n_cols;
                a.kvq_block = 32, a.kvq_cols = t.n_cols;
            } else {
                const auto& t = ops[h.att].u.attention;
                const auto &ks = ops[m.sk].u.slice_assign, &vs = ops[m.sv].u.slice_assign;
                a.att = make_attention(p, t, h.att);
                a.q_rot = buf_at(p, t.q, t.q_off);
                if (!a.att.mask) a.att.mask = p->zero_word, a.att.mask_rs = 0, a.att.mask_cs = 0;
                a.k_cache = p->bufs[ks.dst], a.v_cache = p->bufs[vs.dst];
                a.v_src = buf_at(p, vs.src, vs.src_offset);
                a.k_off = t.k_off, a.v_off = t.v_off;
                a.max_kv = p->sched.bounds[h.att].max_seq_kv ? p->sched.bounds[h.att].max_seq_kv : t.seq_kv;
            }
            if (h.row_store >= 0) {
                const auto& sa = ops[h.row_store].u.slice_assign;
                a.att.dst2 = p->bufs[sa.dst];
                a.att.dyn_dst2_off = p->dyn_dev + h.row_store;
                a.att.d2_rs = sa.dst_row_stride, a.att.d2_cs = sa.dst_col_stride;
            }
            a.q_src = buf_at(p, qr.src, qr.src_off), a.q_cs = buf_at(p, qr.cos_sin, qr.cs_off);
            a.k_src = buf_at(p, kr.src, kr.src_off), a.k_cs = buf_at(p, kr.cos_sin, kr.cs_off);
            a.k_rot = buf_at(p, kr.dst, kr.dst_off);
            a.dyn_k_off = p->dyn_dev + m.sk, a.dyn_v_off = p->dyn_dev + m.sv; // column indices
            a.owner = first_head ? 1 : 0;
            if (sw().hip_attn_trace && first_head && (a.trace = mapped_trace(kAttnTraceWords))) p->attn_traces.push_back(a.trace); // one record per launch
            first_head = false;
            by_dh[a.att.d_head | (m.kvq ? 0x10000u : 0u)].push_back(a);
        }
    }

    // ---- per dependency level of the macro-ops: batches of the plain ops, the chains, the decode-attention launches and the
    // grouped mat-vecs
    void emit_levels() {
        std::sort(macros.begin(), macros.end(), [](const Macro& a, const Macro& b) { return a.position < b.position; });
        std::vector<OpAccess> macro_access(macros.size());
        std::vector<uint64_t> position(macros.size());
        for (size_t i = 0; i < macros.size(); i++) macro_access[i] = macros[i].access, position[i] = macros[i].position;
        std::vector<uint32_t> level;
        std::vector<std::vector<uint32_t>> levels;
        levels_from_access(macro_access, position, p->barriers, level, levels);

        for (const auto& lv : levels) {
            std::vector<PlanItem> plain_ops;
            std::vector<Launch> chains; // the items of a level are mutually independent: their order is free
            std::vector<const Macro*> qmvs;
            std::map<uint32_t, std::vector<AttnDecodeParams>> adec_by_dh; // one launch per head size
            uint32_t adec_lo = UINT32_MAX, adec_hi = 0, adec_ops = 0;
            for (uint32_t mi : lv) {
                const Macro& m = macros[mi];
                if (!m.heads.empty()) {
                    decode_records(m, adec_by_dh);
                    adec_lo = std::min(adec_lo, m.members.front()), adec_hi = std::max(adec_hi, m.members.back());
                    adec_ops += (uint32_t)m.members.size();
                    continue;
                }
                if (m.chain) {
                    const auto& rn = ops[m.anchor].u.rmsnorm;
                    RowChainParams rc;
                    rc.src = buf_at(p, rn.src, rn.src_offset), rc.norm_dst = buf_at(p, rn.dst, rn.dst_offset), rc.cols = rn.cols, rc.eps = rn.eps;
                    if (m.chain_add >= 0) {
                        const auto& e = ops[m.chain_add].u.elementwise;
                        rc.a0 = buf_at(p, e.src0, e.src0_offset), rc.a1 = buf_at(p, e.src1, e.src1_offset), rc.add_dst = buf_at(p, e.dst, e.dst_offset);
                    }
                    if (m.chain_mul >= 0) {
                        const auto& e = ops[m.chain_mul].u.elementwise;
                        const bool norm_is_s0 = e.src0 == rn.dst && e.src0_offset == rn.dst_offset;
                        rc.mul_other = norm_is_s0 ? buf_at(p, e.src1, e.src1_offset) : buf_at(p, e.src0, e.src0_offset);
                        rc.mul_dst = buf_at(p, e.dst, e.dst_offset);
                    }
                    const uint32_t rows = rn.rows;
                    auto rcp = std::make_shared<RowChainParams>(rc); // shared: a later matmul may arm its A-piece output
                    Launch L{ZGML_DOP_RMSNORM, (uint32_t)m.members.size(), m.members.front(), m.members.back(),
                             [=](hipStream_t s) { launch_row_chain(s, *rcp, rows); }};
                    L.hook = std::make_shared<SplitHook>(SplitHook{rcp->mul_dst ? rcp->mul_dst : rcp->norm_dst, rows, rcp->cols, 0, &rcp->ap, &rcp->ap_S, nullptr});
                    L.rc_desc = rcp, L.rc_rows = rows;
                    chains.push_back(std::move(L));
                    continue;
                }
                if (m.elt_chain) {
                    auto ecp = std::make_shared<EltChainParams>(m.elt); // shared: a later matmul may arm its A-piece output
                    Launch L{ZGML_DOP_FUSED_ELEMENTWISE, (uint32_t)m.members.size(), m.members.front(), m.members.back(),
                             [=](hipStream_t s) { launch_eltwise_chain(s, *ecp); }};
                    if (ecp->n_steps && ecp->steps[ecp->n_steps - 1].store)
                        L.hook = std::make_shared<SplitHook>(SplitHook{ecp->steps[ecp->n_steps - 1].store, 0, 0, ecp->n, &ecp->ap, &ecp->ap_S, &ecp->ap_cols});
                    chains.push_back(std::move(L));
                    continue;
                }
                if (m.qmv)
                    qmvs.push_back(&m);
                else if (m.store >= 0)
                    plain_ops.push_back({m.anchor, m.store});
                else
                    plain_ops.push_back({m.members[0], -1});
            }
            emit_batches(p, plain_ops);
            for (Launch& c : chains) p->plan.push_back(std::move(c));
            for (auto& kv : adec_by_dh) {
                const AttnDecodeParams* d = upload_params(p, kv.second);
                const uint32_t nh = (uint32_t)kv.second.size(), dh = kv.first & 0xFFFFu;
                const bool kvq = (kv.first & 0x10000u) != 0; // quantised-KV heads launch on their own
                uint32_t max_kv = 0;
                for (const auto& a : kv.second) max_kv = std::max(max_kv, a.max_kv);
                const AttnSplit sp = attn_split_for(p, nh, dh, max_kv, dh == 128 && !kvq ? 64 : 128);
                Launch AL{ZGML_DOP_ATTENTION, adec_ops, adec_lo, adec_hi, [=](hipStream_t s) { launch_attention_decode_batch(s, d, nh, dh, sp, kvq); }};
                AL.adec_desc = std::make_shared<AdecDesc>(AdecDesc{kv.second, d, nh, dh, sp, kvq});
                p->plan.push_back(std::move(AL));
                adec_ops = 0; // profile accounting: ops counted once
            }
            emit_matvecs(qmvs);
        }
    }

    // mat-vecs of one level that stage the same vector share one launch
    void emit_matvecs(const std::vector<const Macro*>& qmvs) {
        std::vector<char> used(qmvs.size(), 0);
        for (size_t i = 0; i < qmvs.size(); i++) {
            if (used[i]) continue;
            QmvLaunch L;
            std::vector<const Macro*> grp;
            const Macro* first = qmvs[i];
            const QWeightDev& w0 = p->qweights[ops[first->anchor].u.qmatmul.weight_idx];
            for (size_t j = i; j < qmvs.size() && grp.size() < (size_t)kMaxQmvParts; j++) {
                if (used[j]) continue;
                const Macro* c = qmvs[j];
                const QWeightDev& wj = p->qweights[ops[c->anchor].u.qmatmul.weight_idx];
                if (c->pro_sig[0] != first->pro_sig[0] || c->pro_sig[1] != first->pro_sig[1] || c->pro_sig[2] != first->pro_sig[2]) continue;
                if (!qmv_can_group(w0, wj)) continue;
                used[j] = 1;
                grp.push_back(c);
            }
            L.n_parts = (uint32_t)grp.size();
            L.K = w0.K;
            L.pro = first->pro;
            L.pro.store_mid = nullptr, L.pro.store_x = nullptr;
            uint32_t lo = UINT32_MAX, hi = 0, n_ops = 0;
            for (size_t k = 0; k < grp.size(); k++) {
                const Macro* c = grp[k];
                const auto& q = ops[c->anchor].u.qmatmul;
                L.parts[k].w = p->qweights[q.weight_idx];
                L.parts[k].dst = buf_at(p, q.dst, q.dst_offset);
                L.parts[k].n_epi = c->n_epi;
                for (uint32_t e = 0; e < c->n_epi; e++) L.parts[k].epi[e] = c->epi[e];
                if (c->owns_prologue) L.pro.store_mid = c->pro.store_mid, L.pro.store_x = c->pro.store_x;
                lo = std::min(lo, c->members.front());
                hi = std::max(hi, c->members.back());
                n_ops += (uint32_t)c->members.size();
            }
            if (sw().hip_qmv_trace && (L.trace = mapped_trace(16))) // (kind as planned: arm_prenorm / arm_pair may still rewrite it)
                p->qmv_traces.push_back({L.trace, L.n_parts, L.pro.kind, (uint32_t)w0.K, (uint32_t)w0.N});
            auto desc = std::make_shared<QmvLaunch>(L); // shared with the launch: arm_prenorm may still rewrite it
            Launch QL{ZGML_DOP_QMATMUL, n_ops, lo, hi, [desc](hipStream_t s) { launch_qmatvec_fused(s, *desc); }};
            QL.qmv_desc = desc;
            p->plan.push_back(std::move(QL));
        }
    }
};

// The batched plan: the fusion passes in their order (each claims what the ones before it left), the launches level by level,
// then the passes over the launch list (each rewrites launches the next one inspects).
void build_fused_plan(zgml_hip_program* p) {
    Planner pl(p);
    pl.hoist_constant_repeats();
    pl.prologues();
    pl.matvec_macros();
    pl.decode_attention(false);
    pl.decode_attention(true);
    pl.store_folds();
    pl.row_chains();
    pl.elementwise_chains();
    pl.singletons();
    pl.emit_levels();
    fuse_ksplit(p);
    arm_prenorm(p);
    arm_pair(p);
    fuse_qkv_attention(p);
}

} // namespace

namespace zgml_rt {

void free_param_blobs(zgml_hip_program* p) {
    for (void* d : p->param_blobs) hipFree(d);
    p->param_blobs.clear();
}

void build_plan(zgml_hip_program* p) {
    { // a rebuild synchronises the stream and may launch (hoisted repeats): never inside a caller's stream capture (ADVICE r03 — a
      // first upload to a hoist-guarded buffer, or a fusion time-out, can mark the plan dirty between two enqueue calls)
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(p->ctx->stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone) {
            p->ctx->fail("build_plan: the plan has to be rebuilt, but the context's stream is being captured — run one step outside the capture first");
            return;
        }
    }
    hipStreamSynchronize(p->ctx->stream); // the previous plan's parameter arrays may still be in use
    p->plan.clear();
    for (size_t i = 0; i < p->ops.size(); i++) { // (refresh_program refuses this already; a launch must never be skipped silently)
        const zgml_device_op& op = p->ops[i];
        if (op.kind == ZGML_DOP_QMATMUL && op.u.qmatmul.M != 1 && op.u.qmatmul.M > p->kon_max_m && op.u.qmatmul.weight_idx < p->qweights.size() &&
            p->qweights[op.u.qmatmul.weight_idx].format == QW_Q4K)
            p->ctx->fail("build_plan: op " + std::to_string(i) + " is an M > " + std::to_string(p->kon_max_m) + " qmatmul over a weight packed for M <= " +
                         std::to_string(p->kon_max_m) + " mat-vecs (K-on-lanes layout)");
    }
    free_param_blobs(p);
    for (void* d : p->fuse_owned) hipFree(d); // hand-off blocks (granules + generation words, or counters / seen / idx) of the previous plan's fused launches
    p->fuse_owned.clear();
    p->fuse_epoch = p->ctx->fuse_epoch;
    p->split_buf = nullptr, p->split_cnt = nullptr, p->split_buf_floats = 0, p->split_cnt_words = 0; // lived in the blobs
    p->split_pos = UINT64_MAX - 1, p->split_input = nullptr, p->qmm_group = nullptr, p->f16_group = nullptr;
    p->plan_batched = p->ctx->opt_fusion && p->batching_safe;
    if (p->plan_batched) {
        p->sched = build_schedule(p->ops, p->sizes, p->barriers, &p->seq_kv_bound);
        if (!dynamic_fields_in_bounds(p->sched, p->ops)) p->plan_batched = false;
    }
    if (p->plan_batched) {
        build_fused_plan(p);
    } else {
        p->hoist_op.clear(); // op by op: every repeat runs
        for (uint32_t i = 0; i < p->ops.size(); i++) emit_batches(p, {PlanItem{i, -1}});
    }
    p->plan_dirty = false;
    if (sw().hip_debug_plan.set) {
        uint64_t by_kind[ZGML_DOP_COUNT] = {0}, ops_by_kind[ZGML_DOP_COUNT] = {0};
        for (const auto& L : p->plan)
            if (L.kind < ZGML_DOP_COUNT) by_kind[L.kind]++, ops_by_kind[L.kind] += L.n_ops;
        fprintf(stderr, "[zgml_hip] plan: %zu launches for %zu ops (batched=%d):", p->plan.size(), p->ops.size(), (int)p->plan_batched);
        for (int k = 0; k < ZGML_DOP_COUNT; k++)
            if (by_kind[k]) fprintf(stderr, " kind%d=%llu(%llu ops)", k, (unsigned long long)by_kind[k], (unsigned long long)ops_by_kind[k]);
        fprintf(stderr, "\n");
    }
}

} // namespace zgml_rt
