"""CPU tests of the batched decode program over per-sequence int8 KV caches (build_batch_decode_program's kv_quant_block parameter,
zgml_amd/host/llama_decode.hpp) on the oracle: sequence b's logits row is BIT-identical to an independent single-sequence session
with cfg.kv_quant_block = 32 fed the same tokens (the batched plan uses the same kvq_store / attention_kvq ops on the sequence's own
caches); the plan's kv_lanes table; and the column quantisation of zgml_amd/csrc/kvq.h, compiled alone for the CPU, against the
oracle's kvq_store to the bit."""
import copy
import subprocess
from pathlib import Path

import numpy as np
import pytest

from zgml_amd import DeviceOp, DeviceProgram, ProgramIO, capi, llama

KIND = capi.DOP
ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32


def _cfg(kvq=0, **kw):
    cfg = llama.preset("tiny")  # d_head = 32: one block per column
    cfg.kv_quant_block = kvq
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _cfg64():
    """the tiny model with two heads of 64 dims (two blocks per column) and one kv head"""
    return _cfg(n_heads=2, n_kv_heads=1)


def _first_tokens(B, vocab):
    return [(37 * b + 3) % vocab for b in range(B)]


def _run_against_singles(oracle, cfg, kind, B, n_steps, restart=None):
    fns = oracle.backend_fns()
    bm = llama.BatchModel(cfg, B, kind, kv_quant_block=32)
    bs = llama.BatchSession(bm, fns, B)
    cfg1 = copy.copy(cfg)
    cfg1.kv_quant_block = 32
    singles = [llama.Model(cfg1, kind) for _ in range(B)]
    sess = [llama.Session(m, fns) for m in singles]
    toks, pos = np.array(_first_tokens(B, cfg.vocab_size)), np.zeros(B, np.int64)
    for step in range(n_steps):
        if restart and step == restart[0]:
            toks[restart[1]], pos[restart[1]] = restart[2], 0
        nxt, logits = bs.step(toks, pos)
        for b in range(B):
            n1, l1 = sess[b].step(int(toks[b]), int(pos[b]))
            assert np.array_equal(logits[b], l1), (step, b, float(np.abs(logits[b] - l1).max()))
            assert int(nxt[b]) == n1
        toks, pos = nxt.copy(), pos + 1
    bs.close(), bm.close()
    for s, m in zip(sess, singles):
        s.close(), m.close()
    return pos


@pytest.mark.parametrize("B", [2, 3, 5])
@pytest.mark.parametrize("kind", [llama.Q4_0, llama.Q8_0])
def test_int8_rows_are_bit_identical_to_independent_int8_sessions(oracle, kind, B):
    _run_against_singles(oracle, _cfg(), kind, B, 10)


def test_int8_rows_two_blocks_per_column(oracle):
    _run_against_singles(oracle, _cfg64(), llama.Q4_0, 3, 6)


def test_ragged_positions_one_sequence_restarts(oracle):
    """At step 4 sequence 1 starts over at position 0 while the others continue: every kvq_store column and attention_kvq seq_kv
    follows its own sequence's position, and the restarted sequence's stale columns sit behind its own mask column."""
    pos = _run_against_singles(oracle, _cfg(), llama.Q4_0, 3, 9, restart=(4, 1, 411))
    assert pos.tolist() == [9, 5, 9]


def test_patch_batch_moves_the_kvq_fields_per_sequence():
    cfg, B = _cfg(), 3
    bm = llama.BatchModel(cfg, B, kv_quant_block=32)
    toks, pos = [7, 300, 12], [5, 0, 9]
    bm.patch_batch(toks, pos)
    prog = bm.program
    idx, seq = bm.dyn_sequences()
    H, KV, L = cfg.n_heads, cfg.n_kv_heads, cfg.n_layers
    assert idx.size == B * (2 * KV + H) * L and sorted(set(seq.tolist())) == list(range(B))
    lanes = [{lane.buf for lane in bm.kv_lanes(b)} for b in range(B)]
    for i, b in zip(idx.tolist(), seq.tolist()):
        op = prog.ops[i]
        if op.kind == KIND["kvq_store"]:
            st = op.u.kvq_store
            assert st.patch_stride == 1 and st.col == pos[b] and st.col_base == 0 and st.n_cols == cfg.max_seq_len
            assert st.cache in lanes[b] and st.block_size == 32 and st.d_head == cfg.d_head
        else:
            a = op.u.attention_kvq
            assert op.kind == KIND["attention_kvq"] and a.seq_kv == pos[b] + 1 and a.seq_q == 1
            assert a.mask_off == b * cfg.max_seq_len and a.k in lanes[b] and a.v in lanes[b] and a.k != a.v
    assert not any(prog.ops[i].kind in (KIND["attention"],) for i in range(prog.n_ops))
    bm.close()


def _lanes(m, seq=None):
    return [(l.buf, l.offset, l.d_head, l.n_cols, l.block_size) for l in m.kv_lanes(seq)]


def test_kv_lanes_count_order_and_extents():
    cfg, B = _cfg(), 3
    L, KV, dh, S = cfg.n_layers, cfg.n_kv_heads, cfg.d_head, cfg.max_seq_len
    sizes = lambda m: [m.program.buffer_sizes[i] for i in range(m.program.n_buffer_sizes)]
    plain, pre = llama.Model(cfg), llama.Model(cfg, token_len=4)
    plain8 = llama.Model(_cfg(32))
    bf, b8 = llama.BatchModel(cfg, B), llama.BatchModel(cfg, B, kv_quant_block=32)
    for m, n_seq in ((plain, 1), (pre, 1), (plain8, 1), (bf, B), (b8, B)):
        lanes, sz = _lanes(m), sizes(m)
        assert len(lanes) == n_seq * L * KV * 2
        assert lanes == [x for s in range(n_seq) for x in _lanes(m, s)]  # sequence is the outermost index
        for buf, off, d, n_cols, blk in lanes:
            assert d == dh and n_cols == S
            if blk == 0:
                assert off + n_cols * d <= sz[buf]
            else:
                assert blk == 32 and off == 0 and n_cols * d // 4 + n_cols * d // 32 <= sz[buf]
    # f32 plans: (layer, kv head, K | V) inside the consolidated caches
    want = [(plain.buf(w, l), kv * S * dh, dh, S, 0) for l in range(L) for kv in range(KV) for w in ("k_cache", "v_cache")]
    assert _lanes(plain) == want
    assert _lanes(pre) == [(pre.buf(w, l), kv * S * dh, dh, S, 0) for l in range(L) for kv in range(KV) for w in ("k_cache", "v_cache")]
    # batched f32: sequence b's lanes lie in slab b
    slab = bf.kv_slab_elems()
    for b in range(B):
        assert _lanes(bf, b) == [(bf.buf(w, l), b * slab + kv * S * dh, dh, S, 0) for l in range(L) for kv in range(KV) for w in ("k_cache", "v_cache")]
    # int8 plans: one buffer per lane, all distinct, in kv_buffers' order for the single-sequence plan
    for m in (plain8, b8):
        bufs = [x[0] for x in _lanes(m)]
        assert len(set(bufs)) == len(bufs) and all(x[4] == 32 for x in _lanes(m))
        assert sorted(bufs) == sorted(buf for buf, _ in m.kv_buffers())
    assert [x[0] for x in _lanes(plain8)] == [buf for buf, _ in plain8.kv_buffers()]
    with pytest.raises(ValueError):
        bf.kv_lanes(B)
    for m in (plain, pre, plain8, bf, b8):
        m.close()


def test_new_refusals_and_the_pinned_one():
    with pytest.raises(ValueError, match=r"int8 KV.*kv_quant_block"):
        llama.BatchModel(_cfg(32), 2)
    with pytest.raises(ValueError, match=r"int8 KV.*kv_quant_block"):
        llama.BatchModel(_cfg(32), 2, kv_quant_block=32)
    with pytest.raises(ValueError, match="kv_quant_block must be 0 or 32"):
        llama.BatchModel(_cfg(), 2, kv_quant_block=16)
    with pytest.raises(ValueError, match="kv_quant_block must be 0 or 32"):
        llama.BatchModel(_cfg(n_heads=8, n_kv_heads=2), 2, kv_quant_block=32)  # d_head 16
    base = llama.Model(_cfg())
    twin = llama.BatchModel(None, 2, like=base, kv_quant_block=32)
    assert all(l.block_size == 32 for l in twin.kv_lanes())
    twin.close(), base.close()


# ── kvq.h on the CPU ─────────────────────────────────────────────────────────────────────────
def kvq_probe():
    src, exe = ROOT / "tests" / "cpp" / "kvq_probe.cpp", ROOT / "tests" / "cpp" / "_build" / "kvq_probe"
    hdr = ROOT / "zgml_amd" / "csrc" / "kvq.h"
    exe.parent.mkdir(parents=True, exist_ok=True)
    if not exe.exists() or any(s.stat().st_mtime > exe.stat().st_mtime for s in (src, hdr)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-o", str(exe), str(src)], check=True)
    return exe


def probe_quantise(cols, tmp_path):
    """cols [n, d_head] f32 -> (int8 [n, d_head], f32 scales [n, d_head / 32]) through tests/cpp/kvq_probe.cpp"""
    n, dh = cols.shape
    fin, fout = tmp_path / "cols.f32", tmp_path / "cache.bin"
    np.ascontiguousarray(cols, f32).tofile(fin)
    subprocess.run([str(kvq_probe()), str(dh), str(n), str(fin), str(fout)], check=True)
    raw = np.fromfile(fout, np.uint8)
    assert raw.size == n * dh + 4 * n * (dh // 32)
    return raw[:n * dh].view(np.int8).reshape(n, dh), raw[n * dh:].view(f32).reshape(n, dh // 32)


def edge_columns(dh, rng):
    """random columns, then the cases a quantiser gets wrong: an all-zero block, the maximum at both signs, values whose scaled
    magnitude is exactly 127, subnormal magnitudes, and values a hair inside / outside the truncation steps"""
    cols = [((rng.random(dh) - 0.5) * 2 * 10.0 ** rng.integers(-3, 4)).astype(f32) for _ in range(12)]
    z = cols[0].copy()
    z[:32] = 0.0
    cols.append(z)
    cols.append(np.zeros(dh, f32))
    both = cols[1].copy()
    both[3], both[17] = 7.25, -7.25
    both[np.abs(both) > 7.25] *= 0.01
    cols.append(both)
    exact = (np.arange(dh) % 255 - 127).astype(f32)  # max 127: inv = 1, every value an integer
    exact[0], exact[1] = 127.0, -127.0
    cols.append(exact)
    cols.append((exact * f32(0.3)).astype(f32))
    sub = (rng.integers(-127, 128, dh) * np.float32(1e-45)).astype(f32)  # multiples of the smallest subnormal
    sub[5] = np.float32(127 * 1.4e-45)
    cols.append(sub)
    cols.append(np.full(dh, np.float32(1.1754942e-38), f32) * np.where(np.arange(dh) % 2, 1, -1).astype(f32))  # largest subnormal
    steps = (np.arange(dh) % 127 + 1).astype(f32)
    steps[0] = 127.0
    cols.append(np.nextafter(steps, f32(0)).astype(f32))
    cols.append(np.nextafter(steps[::-1].copy(), f32(200)).astype(f32))
    return np.stack(cols)


@pytest.mark.parametrize("dh", [32, 64, 128, 256])
def test_kvq_header_equals_the_oracles_kvq_store(oracle, tmp_path, dh):
    cols = edge_columns(dh, np.random.default_rng(dh))
    n = cols.shape[0]
    q, sc = probe_quantise(cols, tmp_path)
    ce = n * dh // 4 + n * (dh // 32)
    prog = DeviceProgram(ops=[DeviceOp.kvq_store(0, 1, dh, 32, n, c * dh, 0, c, 1) for c in range(n)], buffer_sizes=[ce, n * dh],
                         initial_uploads=[ProgramIO(1, cols.ravel())])
    cache = oracle.run_program(prog, 0, ce)
    want_q = cache[:n * dh // 4].view(np.int8).reshape(n, dh)
    want_sc = cache[n * dh // 4:].reshape(n, dh // 32)
    assert np.array_equal(q, want_q)
    assert np.array_equal(sc.view(np.uint32), want_sc.view(np.uint32))
    assert not cols[13].any() and np.all(sc[13] == 1.0) and not q[13].any()  # the all-zero column: scale 1, quants 0
    assert np.abs(q).max() == 127
