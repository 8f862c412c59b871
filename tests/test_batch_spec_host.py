"""CPU tests of the B x Ts batched plan (build_batch_decode_program's tokens_per_seq, zgml_amd/host/llama_decode.hpp) on the oracle:
one step runs Ts consecutive positions of each of B independent sequences — the verify step of
zgml_hip_resident_decode_batch_speculative — and EVERY logits row of it is BIT-identical to the corresponding row of an independent
token_len = Ts session fed the same tokens at the same positions (the rule of tests/test_batch_decode_host.py: the step is written in
the existing DeviceOps, and the oracle computes a row the same way whatever M is). The steps are ragged as a verify loop's are:
every sequence advances by its own count, so later steps overlap columns already stored."""
import copy

import numpy as np
import pytest

from zgml_amd import capi, llama

KIND = capi.DOP
CASES = [(2, 2), (3, 4), (2, 5)]


def _cfg(**kw):
    cfg = llama.preset("tiny")
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _token(b, pos, salt, vocab):
    return (37 * b + 11 * pos + 5 * salt + 3) % vocab


def _rows_against_singles(oracle, kind, B, Ts, kvq):
    cfg = _cfg()
    fns, ob = oracle.backend_fns(), oracle.OracleBackend()
    bm = llama.BatchModel(cfg, B, kind, kv_quant_block=kvq, tokens_per_seq=Ts)
    bs = llama.BatchSession(bm, fns, B)
    assert bs.tokens_per_seq == Ts and bm.token_len == B * Ts and bm.lib.zh_model_tokens_per_seq(bm.ptr) == Ts
    cfg1 = copy.copy(cfg)
    cfg1.kv_quant_block = kvq
    singles = [llama.Model(cfg1, kind, token_len=Ts) for _ in range(B)]
    sess = [llama.Session(m, fns) for m in singles]
    V = cfg.vocab_size
    pos = [3 * b for b in range(B)]  # ragged from the start (columns in front of a start are masked for both sides alike)
    for step in range(5):
        toks = [_token(b, pos[b] + j, step, V) for b in range(B) for j in range(Ts)]
        nxt, logits = bs.step(toks, pos)
        assert logits.shape == (B * Ts, V) and nxt.shape == (B * Ts,)
        for b in range(B):
            last, l_last = sess[b].prefill(toks[b * Ts:(b + 1) * Ts], pos[b])
            rows = ob.buffer(sess[b].handle, singles[b].buf("logits"))[:Ts * V].reshape(Ts, V)
            assert np.array_equal(rows[Ts - 1], l_last)
            for j in range(Ts):
                got = logits[b * Ts + j]
                assert np.array_equal(got, rows[j]), (step, b, j, float(np.abs(got - rows[j]).max()))
                assert int(nxt[b * Ts + j]) == int(np.argmax(rows[j]))
        pos = [pos[b] + 1 + (step + b) % Ts for b in range(B)]  # every sequence advances by its own count, 1..Ts
    bs.close(), bm.close()
    for s, m in zip(sess, singles):
        s.close(), m.close()


@pytest.mark.parametrize("B,Ts", CASES)
@pytest.mark.parametrize("kind", [llama.Q4_0, llama.Q8_0])
def test_every_row_is_bit_identical_to_independent_token_len_sessions(oracle, kind, B, Ts):
    _rows_against_singles(oracle, kind, B, Ts, 0)


@pytest.mark.parametrize("B,Ts", CASES)
@pytest.mark.parametrize("kind", [llama.Q4_0, llama.Q8_0])
def test_int8_rows_are_bit_identical_to_independent_int8_sessions(oracle, kind, B, Ts):
    _rows_against_singles(oracle, kind, B, Ts, 32)


@pytest.mark.parametrize("B,Ts", CASES)
def test_patch_batch_fields_per_sequence(B, Ts):
    cfg = _cfg()
    bm = llama.BatchModel(cfg, B, tokens_per_seq=Ts)
    S, dh, H, KV, L = cfg.max_seq_len, cfg.d_head, cfg.n_heads, cfg.n_kv_heads, cfg.n_layers
    pos = [5, 0, 9][:B]
    bm.patch_batch([(7 * i + 1) % cfg.vocab_size for i in range(B * Ts)], pos)
    prog = bm.program
    idx, seq = bm.dyn_sequences()
    assert idx.size == B * (2 * KV + H) * L and sorted(set(seq.tolist())) == list(range(B))
    slab = bm.kv_slab_elems()
    for i, b in zip(idx.tolist(), seq.tolist()):
        op = prog.ops[i]
        if op.kind == KIND["slice_assign"]:
            sa = op.u.slice_assign
            assert sa.patch_stride != 0 and sa.cols == Ts
            assert sa.dst_offset == sa.dst_base_offset + pos[b] * sa.patch_stride  # stores at base + pos[b] * stride ...
            assert b * slab <= sa.dst_base_offset and sa.dst_base_offset + (S - 1) * sa.patch_stride < (b + 1) * slab  # ... inside b's slab
        else:
            a = op.u.attention
            assert op.kind == KIND["attention"] and a.seq_kv == pos[b] + Ts and a.seq_q == Ts
            assert a.mask_off == b * Ts * S and b * slab <= a.k_off < (b + 1) * slab and a.k_off == a.v_off
    ropes = [prog.ops[i].u.rope for i in range(prog.n_ops) if prog.ops[i].kind == KIND["rope"]]
    assert len(ropes) == B * (H + KV) * L and all(r.seq_len == Ts for r in ropes)
    assert sorted({r.cs_off for r in ropes}) == [b * Ts * 2 * dh for b in range(B)]
    qm = [prog.ops[i].u.qmatmul for i in range(prog.n_ops) if prog.ops[i].kind == KIND["qmatmul"]]
    assert len(qm) == 7 * L and all(q.M == B * Ts for q in qm)
    # the row stores (patch_stride 0) put sequence b's heads into its own Ts columns
    stores = [prog.ops[i].u.slice_assign for i in range(prog.n_ops) if prog.ops[i].kind == KIND["slice_assign"] and prog.ops[i].u.slice_assign.patch_stride == 0]
    assert sorted({s.dst_offset // (Ts * cfg.d_model) for s in stores}) == list(range(B)) and all(s.cols == Ts for s in stores)
    bm.close()


def test_patch_batch_int8_columns_per_sequence():
    cfg, B, Ts = _cfg(), 2, 4
    bm = llama.BatchModel(cfg, B, kv_quant_block=32, tokens_per_seq=Ts)
    pos = [6, 1]
    bm.patch_batch([3] * (B * Ts), pos)
    prog = bm.program
    idx, seq = bm.dyn_sequences()
    lanes = [{lane.buf for lane in bm.kv_lanes(b)} for b in range(B)]
    cols = {b: [] for b in range(B)}
    for i, b in zip(idx.tolist(), seq.tolist()):
        op = prog.ops[i]
        if op.kind == KIND["kvq_store"]:
            st = op.u.kvq_store
            assert st.cache in lanes[b] and st.col == st.col_base + pos[b] and st.patch_stride == 1
            cols[b].append(st.col)
        else:
            a = op.u.attention_kvq
            assert op.kind == KIND["attention_kvq"] and a.seq_kv == pos[b] + Ts and a.seq_q == Ts and a.mask_off == b * Ts * cfg.max_seq_len
            assert a.k in lanes[b] and a.v in lanes[b]
    for b in range(B):  # one store per column and cache: the Ts columns from pos[b]
        assert sorted(set(cols[b])) == list(range(pos[b], pos[b] + Ts))
        assert len(cols[b]) == Ts * 2 * cfg.n_kv_heads * cfg.n_layers
    bm.close()


def _op_list(prog):
    """every op as (kind, the bytes of its own member of the union) — a fused_elementwise op, whose member holds a pointer, as its
    counts and buffers — and the buffer sizes"""
    import ctypes as C
    names = {v: k for k, v in KIND.items()}
    out = []
    for i in range(prog.n_ops):
        op = prog.ops[i]
        member = getattr(op.u, names[op.kind])
        if names[op.kind] == "fused_elementwise":
            out.append((op.kind, tuple(getattr(member, f) for f, *_ in member._fields_ if "step" not in f or f.startswith("n_"))))
        else:
            out.append((op.kind, C.string_at(C.addressof(member), C.sizeof(member))))
    return out, [prog.buffer_sizes[i] for i in range(prog.n_buffer_sizes)]


@pytest.mark.parametrize("kvq", [0, 32])
def test_one_token_per_sequence_is_todays_program(kvq):
    """tokens_per_seq = 1, said or not, gives the same op list: and it is the list the single-column builder has always made, whose
    shape tests/test_batch_decode_host.py pins field by field"""
    cfg, B = _cfg(), 3
    a, b = llama.BatchModel(cfg, B, kv_quant_block=kvq), llama.BatchModel(cfg, B, kv_quant_block=kvq, tokens_per_seq=1)
    assert a.tokens_per_seq == 1 and a.token_len == B
    assert _op_list(a.program) == _op_list(b.program)
    import ctypes as C
    err = C.create_string_buffer(256)
    old = a.lib.zh_model_create_batch_kvq(C.byref(cfg), llama.Q4_0, 1, 0, 8, B, kvq, err, len(err))  # the entry point without the parameter
    assert old, err.value
    assert _op_list(a.lib.zh_model_program(old).contents) == _op_list(a.program)
    a.lib.zh_model_free(old)
    ops = [a.program.ops[i] for i in range(a.program.n_ops)]
    att = [o for o in ops if o.kind in (KIND["attention"], KIND["attention_kvq"])]
    assert len(att) == B * cfg.n_heads * cfg.n_layers
    assert all((o.u.attention.seq_q if o.kind == KIND["attention"] else o.u.attention_kvq.seq_q) == 1 for o in att)
    a.close(), b.close()


def test_builder_refuses_tokens_per_seq_outside_1_to_16():
    for ts in (0, 17):
        with pytest.raises(ValueError, match="tokens_per_seq"):
            llama.BatchModel(_cfg(), 2, tokens_per_seq=ts)
    base = llama.Model(_cfg())
    with pytest.raises(ValueError, match="tokens_per_seq"):
        llama.BatchModel(None, 2, like=base, tokens_per_seq=17)
    m = llama.BatchModel(None, 2, like=base, tokens_per_seq=16)
    assert m.token_len == 32
    m.close(), base.close()


def test_new_symbol_is_declared_and_exported():
    name = "zgml_hip_resident_decode_batch_speculative"
    assert name in capi.HIP_SYMBOLS
    if capi.HIP_LIB_PATH.exists():
        assert hasattr(capi.load_hip(), name)
