"""CPU tests of the batched decode program (build_batch_decode_program, zgml_amd/host/llama_decode.hpp) on the oracle: one step
advances B independent sequences, and sequence b's logits row is BIT-identical to an independent single-sequence session fed
the same tokens — the batched step is written in the existing DeviceOps, and the oracle's qmatmul / matmul / norm / elementwise
paths compute a row the same way whatever M is (no op needed the 1e-6 allowance)."""
import numpy as np
import pytest

from zgml_amd import capi, llama

KIND = capi.DOP


def _cfg(tied=True, **kw):
    cfg = llama.preset("tiny")
    cfg.tied_lm_head = int(tied)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _first_tokens(B, vocab):
    return [(37 * b + 3) % vocab for b in range(B)]


@pytest.mark.parametrize("B", [2, 3, 5])
@pytest.mark.parametrize("tied", [True, False])
@pytest.mark.parametrize("kind", [llama.Q4_0, llama.Q8_0])
def test_rows_are_bit_identical_to_independent_sessions(oracle, kind, tied, B):
    cfg = _cfg(tied)
    fns = oracle.backend_fns()
    bm = llama.BatchModel(cfg, B, kind)
    bs = llama.BatchSession(bm, fns, B)
    singles = [llama.Model(cfg, kind) for _ in range(B)]
    sess = [llama.Session(m, fns) for m in singles]
    toks = np.array(_first_tokens(B, cfg.vocab_size))
    pos = np.zeros(B, np.int64)
    for step in range(10):
        nxt, logits = bs.step(toks, pos)
        for b in range(B):
            n1, l1 = sess[b].step(int(toks[b]), int(pos[b]))
            assert np.array_equal(logits[b], l1), (step, b, float(np.abs(logits[b] - l1).max()))
            assert int(nxt[b]) == n1
        toks, pos = nxt.copy(), pos + 1
    bs.close(), bm.close()
    for s, m in zip(sess, singles):
        s.close(), m.close()


def test_ragged_positions_one_sequence_restarts(oracle):
    """At step 4 sequence 1 starts over (position 0, a new first token) while the others continue: every dynamic op follows its own
    sequence's position, and the restarted sequence's stale KV columns sit behind its own mask column."""
    cfg, B = _cfg(), 3
    fns = oracle.backend_fns()
    bs = llama.BatchSession(llama.Model(cfg, llama.Q4_0), fns, B)  # (a plain Model: the session builds the batched twin)
    assert isinstance(bs.model, llama.BatchModel) and bs.model.n_seqs == B
    singles = [llama.Model(cfg, llama.Q4_0) for _ in range(B)]
    sess = [llama.Session(m, fns) for m in singles]
    toks, pos = np.array(_first_tokens(B, cfg.vocab_size)), np.zeros(B, np.int64)
    for step in range(9):
        if step == 4:
            toks[1], pos[1] = 411, 0
        nxt, logits = bs.step(toks, pos)
        for b in range(B):
            n1, l1 = sess[b].step(int(toks[b]), int(pos[b]))
            assert np.array_equal(logits[b], l1), (step, b)
            assert int(nxt[b]) == n1
        toks, pos = nxt.copy(), pos + 1
    assert pos.tolist() == [9, 5, 9]
    bs.close()
    for s, m in zip(sess, singles):
        s.close(), m.close()


def test_patch_batch_writes_columns_and_per_sequence_dynamic_fields():
    cfg, B = _cfg(), 3
    bm = llama.BatchModel(cfg, B)
    toks, pos = [7, 300, 12], [5, 0, 9]
    bm.patch_batch(toks, pos)
    prog = bm.program
    idx, seq = bm.dyn_sequences()
    H, KV, L = cfg.n_heads, cfg.n_kv_heads, cfg.n_layers
    assert idx.size == B * (2 * KV + H) * L and sorted(set(seq.tolist())) == list(range(B))
    slab = bm.kv_slab_elems()
    for i, b in zip(idx.tolist(), seq.tolist()):
        op = prog.ops[i]
        if op.kind == KIND["slice_assign"]:
            sa = op.u.slice_assign
            assert sa.patch_stride != 0 and sa.cols == 1
            assert sa.dst_offset == sa.dst_base_offset + pos[b] * sa.patch_stride
            assert b * slab <= sa.dst_base_offset < (b + 1) * slab  # sequence b's slab
        else:
            a = op.u.attention
            assert op.kind == KIND["attention"] and a.seq_kv == pos[b] + 1 and a.seq_q == 1
            assert a.mask_off == b * cfg.max_seq_len and b * slab <= a.k_off < (b + 1) * slab and a.k_off == a.v_off
    ropes = [prog.ops[i].u.rope for i in range(prog.n_ops) if prog.ops[i].kind == KIND["rope"]]
    assert len(ropes) == B * (H + KV) * L and all(r.seq_len == 1 for r in ropes)
    assert sorted({r.cs_off for r in ropes}) == [b * 2 * cfg.d_head for b in range(B)]
    qm = [prog.ops[i].u.qmatmul for i in range(prog.n_ops) if prog.ops[i].kind == KIND["qmatmul"]]
    assert len(qm) == 7 * L and all(q.M == B for q in qm)
    assert [(buf, n) for buf, n in bm.kv_buffers()] == [(bm.buf(w, l), B * slab) for l in range(L) for w in ("k_cache", "v_cache")]
    bm.close()


def test_single_sequence_prefills_hand_their_caches_to_the_slabs(oracle):
    """B single-sequence prefill plans (prompts of different lengths) fill their caches; copied to b * slab of the batched plan's
    buffers — and to a single-sequence decode plan each — the next batched step equals the independent sessions' next step."""
    cfg, B = _cfg(), 3
    fns, ob = oracle.backend_fns(), oracle.OracleBackend()
    bm = llama.BatchModel(cfg, B)
    bs = llama.BatchSession(bm, fns, B)
    slab = bm.kv_slab_elems()
    toks, pos, dec = [], [], []
    for b in range(B):
        T = 4 + 2 * b
        prompt = [(11 * b + 5 * j + 1) % cfg.vocab_size for j in range(T)]
        mp = llama.Model(cfg, llama.Q4_0, token_len=T)
        sp = llama.Session(mp, fns)
        nxt, _ = sp.prefill(prompt, 0)
        md = llama.Model(cfg, llama.Q4_0)
        sd = llama.Session(md, fns)
        for (src, n), (dst1, n1), (dstb, nb) in zip(mp.kv_buffers(), md.kv_buffers(), bm.kv_buffers()):
            assert n == n1 == slab and nb == B * slab
            img = ob.buffer(sp.handle, src)[:n]
            ob.buffer(sd.handle, dst1)[:n] = img
            ob.buffer(bs.handle, dstb)[b * slab:(b + 1) * slab] = img
        toks.append(nxt), pos.append(T), dec.append((md, sd))
        sp.close(), mp.close()
    for step in range(3):
        nxt, logits = bs.step(toks, pos)
        for b, (md, sd) in enumerate(dec):
            n1, l1 = sd.step(int(toks[b]), int(pos[b]))
            assert np.array_equal(logits[b], l1), (step, b)
            assert int(nxt[b]) == n1
        toks, pos = nxt.tolist(), [p + 1 for p in pos]
    bs.close(), bm.close()
    for md, sd in dec:
        sd.close(), md.close()


def test_builder_refusals():
    with pytest.raises(ValueError, match="int8 KV"):
        llama.BatchModel(_cfg(kv_quant_block=32), 2)
    with pytest.raises(ValueError, match="row shard"):
        llama.BatchModel(_cfg(tied=False, shard_world=2), 2)
    for n in (0, 33):
        with pytest.raises(ValueError, match="n_seqs"):
            llama.BatchModel(_cfg(), n)
    m = llama.BatchModel(_cfg(), 32)
    assert m.n_seqs == 32 and m.lib.zh_model_n_seqs(m.ptr) == 32
    m.close()
