"""Batched decode on the MI355X: one program step advances B independent sequences (build_batch_decode_program), stepped
through the HIP C ABI and through the oracle — logits of every sequence within 2e-4 of that row's logit range with identical
greedy tokens (the bar of tests/test_hip_llama.py) —, the device-resident batched loop, the per-sequence dynamic refresh, the
launch plan's shape and the errors of using a batched program through the single-sequence entry points and vice versa."""
import ctypes as C
import re

import numpy as np
import pytest

from zgml_amd import capi, llama
from tests.test_hip_l7dims import l7cfg

pytestmark = pytest.mark.gpu
TOL = 2e-4


def launches(text):
    out = []
    for line in text.splitlines():
        m = re.match(r"\d+: kind (\d+) ops (\d+) \[(\d+)\.\.(\d+)\](.*)", line)
        assert m, line
        out.append((int(m[1]), int(m[2]), int(m[3]), int(m[4]), m[5]))
    return out


def plan_text(be, handle):
    hip = capi.load_hip()
    n = hip.zgml_hip_program_plan_text(be.ctx, handle, None, 0)
    buf = C.create_string_buffer(int(n) + 1)
    hip.zgml_hip_program_plan_text(be.ctx, handle, buf, n + 1)
    return buf.value.decode()


def step_both(be, oracle, bm, B, tokens, positions, n_steps, small_m=True, ref_trace=None):
    """Step the oracle and HIP sessions over the same BatchModel, feeding both the oracle's greedy tokens. Returns the worst
    |delta| / row range and the oracle's (tokens, positions, logits, next) per step (reusable through `ref_trace`)."""
    s_hip = llama.BatchSession(bm, llama.hip_backend_fns(be), B, small_m_matvec=small_m)
    s_ref = None if ref_trace else llama.BatchSession(bm, oracle.backend_fns(), B)
    toks, pos, worst, trace = np.array(tokens), np.array(positions), 0.0, []
    for step in range(n_steps):
        if ref_trace:
            toks, pos, l_ref, t_ref = ref_trace[step]
        else:
            t_ref, l_ref = s_ref.step(toks, pos)
        t_hip, l_hip = s_hip.step(toks, pos)
        assert not be.last_error(), be.last_error()
        assert np.isfinite(l_hip).all()
        for b in range(B):
            rel = float(np.abs(l_hip[b] - l_ref[b]).max() / np.abs(l_ref[b]).max())
            worst = max(worst, rel)
            assert rel < TOL, (step, b, rel)
        assert t_hip.tolist() == t_ref.tolist(), (step, t_hip, t_ref)
        trace.append((toks.copy(), pos.copy(), l_ref, t_ref))
        toks, pos = t_ref.copy(), pos + 1
    s_hip.close()
    if s_ref:
        s_ref.close()
    return worst, trace


@pytest.mark.parametrize("kind", [llama.Q4_0, llama.Q8_0])
@pytest.mark.parametrize("fused", [True, False])
def test_tiny_batch_matches_oracle(hip_backend, oracle, kind, fused):
    B = 3
    bm = llama.BatchModel(llama.preset("tiny"), B, kind, fused_elementwise=fused, include_dead_f32=True)
    worst, _ = step_both(hip_backend, oracle, bm, B, [3, 40, 77], [0, 5, 2], 12)
    print("worst:", worst)
    bm.close()


def test_tiny_batch_untied_head_and_graph_off(hip_backend, oracle):
    cfg = llama.preset("tiny")
    cfg.tied_lm_head = 0
    B = 3
    bm = llama.BatchModel(cfg, B, llama.Q4_0)
    hip_backend.set_option(capi.OPT_GRAPH, 0)
    try:
        step_both(hip_backend, oracle, bm, B, [3, 40, 77], [0, 0, 0], 12)
    finally:
        hip_backend.set_option(capi.OPT_GRAPH, 1)
    bm.close()


def test_smollm_135m_batch_matches_oracle(hip_backend, oracle):
    oracle.set_threads(16)
    B = 4
    bm = llama.BatchModel(llama.preset("smollm-135m"), B, llama.Q4_0, threads=16)
    worst, _ = step_both(hip_backend, oracle, bm, B, [3, 40, 77, 1001], [0, 1, 7, 3], 4)
    print("worst:", worst)
    bm.close()


@pytest.mark.parametrize("B", [2, 4, 8])
def test_l7_dimensions_small_m_matvec_on_and_off(hip_backend, oracle, B):
    """Llama-2-7B dimensions, two layers: sequence 0 sits past the attention-split threshold (position 300: its heads' context is
    split over several workgroups) while sequence 1 starts at position 0, in the same step and the same attention launch. Option
    on (value 8: every B here): the projections run through the multi-row K-on-lanes mat-vec; off: through the tile kernels."""
    oracle.set_threads(16)
    bm = llama.BatchModel(l7cfg(2), B, llama.Q4_0, threads=16)
    tokens = [(911 * b + 17) % bm.cfg.vocab_size for b in range(B)]
    positions = [300, 0] + [40 * b + 1 for b in range(2, B)]
    worst_on, trace = step_both(hip_backend, oracle, bm, B, tokens, positions, 3, small_m=8)  # (8: the row kernel also at B = 7, 8)
    worst_off, _ = step_both(hip_backend, oracle, bm, B, tokens, positions, 3, small_m=False, ref_trace=trace)
    print("worst on / off:", worst_on, worst_off)
    bm.close()


def stepped_tokens(s, first, start, n_steps):
    """Greedy streams by stepping: sequence b runs n_steps[b] steps; a finished sequence repeats its last step."""
    B = len(first)
    toks, pos, left = np.array(first), np.array(start), np.array(n_steps)
    out = np.full((B, int(max(n_steps))), -1, np.int64)
    for i in range(int(max(n_steps))):
        nxt, _ = s.step(toks, pos)
        for b in range(B):
            if left[b] > 0:
                out[b, i] = nxt[b]
                toks[b], pos[b], left[b] = nxt[b], pos[b] + 1, left[b] - 1
    return out


@pytest.mark.parametrize("name,kind", [("tiny", llama.Q4_0), ("tiny", llama.Q8_0), ("smollm-135m", llama.Q4_0)])
def test_resident_batch_equals_stepping(hip_backend, name, kind):
    B, n = 3, (16 if name == "tiny" else 8)
    bm = llama.BatchModel(llama.preset(name), B, kind, threads=8)
    s = llama.BatchSession(bm, llama.hip_backend_fns(hip_backend), B)
    first, start = [5, 90, 33], [0, 3, 1]
    s.resident_setup(hip_backend)
    got = s.resident_decode_batch(first, start, n)  # the program's first execution is the resident loop
    assert not hip_backend.last_error(), hip_backend.last_error()
    want = stepped_tokens(s, first, start, [n] * B)  # the vtable path after a resident run
    assert got.tolist() == want.tolist()
    # ragged counts: a finished sequence is frozen, the rest of its row stays -1
    counts = [n, n // 2, 1]
    ragged = s.resident_decode_batch(first, start, counts)
    assert ragged.shape == (B, n)
    for b in range(B):
        assert ragged[b, :counts[b]].tolist() == want[b, :counts[b]].tolist() and np.all(ragged[b, counts[b]:] == -1)
    # the frozen sequences' caches are intact: resume every sequence mid-stream on the warm caches
    full = s.resident_decode_batch(first, start, n)
    assert full.tolist() == want.tolist()
    h = n // 2
    resumed = s.resident_decode_batch(want[:, h - 1], [p + h for p in start], n - h)
    assert resumed.tolist() == want[:, h:].tolist()
    again = stepped_tokens(s, first, start, [n] * B)
    assert again.tolist() == want.tolist()
    assert not hip_backend.last_error(), hip_backend.last_error()
    s.close(), bm.close()


def test_resident_batch_refuses_out_of_range_requests(hip_backend):
    B = 2
    cfg = llama.preset("tiny")
    bm = llama.BatchModel(cfg, B)
    s = llama.BatchSession(bm, llama.hip_backend_fns(hip_backend), B)
    s.resident_setup(hip_backend)
    hip = capi.load_hip()
    for first, start, steps in (([cfg.vocab_size, 1], [0, 0], [2, 2]), ([1, 1], [cfg.max_seq_len - 1, 0], [2, 2]),
                                ([1, 1], [cfg.max_seq_len - 2, 0], [2, 4])):  # (the last: it would idle at position max_seq)
        with pytest.raises(RuntimeError, match="out of range"):
            s.resident_decode_batch(first, start, steps)
        hip.zgml_hip_clear_error(hip_backend.ctx)
    ok = s.resident_decode_batch([1, 1], [cfg.max_seq_len - 2, 0], [2, 2])
    assert ok.shape == (B, 2) and np.all(ok >= 0) and not hip_backend.last_error()
    s.close(), bm.close()


def test_dynamic_refresh_batch_equals_full_refresh(hip_backend):
    cfg, B = llama.preset("tiny", 128), 3
    bm = llama.BatchModel(cfg, B)
    s_full = llama.BatchSession(bm, llama.hip_backend_fns(hip_backend), B)
    s_dyn = llama.BatchSession(bm, llama.hip_backend_fns(hip_backend), B)
    s_dyn.use_dynamic_refresh()
    rng = np.random.default_rng(5)
    for step in range(14):
        toks = rng.integers(0, cfg.vocab_size, B)
        pos = [step, (step * 7) % 23, 60 - step]  # every sequence moves on its own, forwards and backwards
        t_f, l_f = s_full.step(toks, pos)
        t_d, l_d = s_dyn.step(toks, pos)
        assert not hip_backend.last_error(), hip_backend.last_error()
        assert t_f.tolist() == t_d.tolist() and np.array_equal(l_f, l_d), step
    s_full.close(), s_dyn.close(), bm.close()


def test_position_outside_the_compiled_bounds_falls_back_to_program_order(hip_backend, oracle):
    """The program is compiled with every attention's seq_kv at 1 (all sequences patched to position 0): the batched plan's level
    schedule assumed that extent, so the first refresh beyond it switches the program to program order for good — with the same
    results, through either refresh."""
    cfg, B = llama.preset("tiny"), 3
    bm = llama.BatchModel(cfg, B)
    bm.patch_batch([1] * B, [0] * B)
    fns = llama.hip_backend_fns(hip_backend)
    s_ref = llama.BatchSession(bm, oracle.backend_fns(), B)
    sessions = [llama.BatchSession(bm, fns, B), llama.BatchSession(bm, fns, B)]
    sessions[1].use_dynamic_refresh()
    batched_before = [len(launches(plan_text(hip_backend, s.handle))) for s in sessions]
    toks, pos = np.array([3, 40, 77]), np.array([0, 0, 0])
    for step in range(6):
        t_ref, l_ref = s_ref.step(toks, pos)
        for s in sessions:
            t, l = s.step(toks, pos)
            assert not hip_backend.last_error(), hip_backend.last_error()
            assert t.tolist() == t_ref.tolist()
            assert max(float(np.abs(l[b] - l_ref[b]).max() / np.abs(l_ref[b]).max()) for b in range(B)) < TOL
        toks, pos = t_ref.copy(), pos + np.array([1, 2, 0])
    for s, before in zip(sessions, batched_before):
        assert before < len(launches(plan_text(hip_backend, s.handle))) <= bm.program.n_ops  # op by op now
    for s in sessions + [s_ref]:
        s.close()
    bm.close()


def test_set_sequences_needs_every_dynamic_op(hip_backend):
    B = 2
    bm = llama.BatchModel(llama.preset("tiny"), B)
    s = llama.BatchSession(bm, llama.hip_backend_fns(hip_backend), B)
    hip, u32p = capi.load_hip(), C.POINTER(C.c_uint32)
    idx, seq = bm.dyn_sequences()
    assert hip.zgml_hip_program_set_sequences(hip_backend.ctx, s.handle, B, idx[1:].ctypes.data_as(u32p), seq[1:].ctypes.data_as(u32p), idx.size - 1) != 0
    err = hip_backend.last_error()
    assert "set_sequences" in err and f"op {idx[0]}" in err, err
    hip.zgml_hip_clear_error(hip_backend.ctx)
    bad = seq.copy()
    bad[0] = B
    assert hip.zgml_hip_program_set_sequences(hip_backend.ctx, s.handle, B, idx.ctypes.data_as(u32p), bad.ctypes.data_as(u32p), idx.size) != 0
    hip.zgml_hip_clear_error(hip_backend.ctx)
    nxt, _ = s.step([1, 2], [0, 0])  # the earlier declaration is still in force
    assert not hip_backend.last_error() and nxt.shape == (B,)
    s.close(), bm.close()


def test_plan_shape_at_7b_dimensions(hip_backend):
    """Per layer, with the option on: row chain; q, k, v; ONE decode-attention launch carrying the B * 32 heads (ropes, K / V stores,
    attention and row store of every head of every sequence folded: 6 ops per head at n_kv = n_heads); o; row chain; gate, up; one
    elementwise chain; down — 11 launches. Then the final norm's row chain and the LM head."""
    B, L = 4, 2
    cfg = l7cfg(L)
    bm = llama.BatchModel(cfg, B, llama.Q4_0, threads=16)
    s = llama.BatchSession(bm, llama.hip_backend_fns(hip_backend), B)
    text = plan_text(hip_backend, s.handle)
    ls = launches(text)
    adec = [l for l in ls if "decode-attention" in l[4]]
    assert len(adec) == L, text
    H, KV = cfg.n_heads, cfg.n_kv_heads
    assert all(l[1] == B * (3 * KV + 3 * H) for l in adec), text
    rows = [l for l in ls if "qmatvec-kon-rows" in l[4]]
    assert len(rows) == 7 * L + 1, text
    K = capi.DOP
    layer = [K["rmsnorm"], K["qmatmul"], K["qmatmul"], K["qmatmul"], K["attention"], K["qmatmul"], K["rmsnorm"], K["qmatmul"], K["qmatmul"],
             K["fused_elementwise"], K["qmatmul"]]
    assert [l[0] for l in ls] == layer * L + [K["rmsnorm"], K["qmatmul"]], text  # 11 launches per layer, then the final norm and the LM head
    s.close(), bm.close()


def test_cross_use_is_refused_without_a_sticky_fault(hip_backend):
    hip = capi.load_hip()
    cfg, B = llama.preset("tiny"), 2
    bm = llama.BatchModel(cfg, B)
    sb = llama.BatchSession(bm, llama.hip_backend_fns(hip_backend), B)
    sb.resident_setup(hip_backend)
    toks = np.zeros(4, np.int64)
    assert hip.zgml_hip_resident_decode(hip_backend.ctx, sb.handle, 1, 0, 4, toks.ctypes.data) != 0
    assert "batched" in hip_backend.last_error()
    hip.zgml_hip_clear_error(hip_backend.ctx)
    two = np.array([1, 2], np.uint32)
    assert hip.zgml_hip_resident_prefill(hip_backend.ctx, sb.handle, two.ctypes.data_as(C.POINTER(C.c_uint32)), 2, 0) < 0
    assert "batched" in hip_backend.last_error()
    hip.zgml_hip_clear_error(hip_backend.ctx)
    m = llama.Model(cfg)
    s1 = llama.Session(m, llama.hip_backend_fns(hip_backend))
    s1.resident_setup(hip_backend)
    u32p = C.POINTER(C.c_uint32)
    one, zero, cnt = np.array([1], np.uint32), np.array([0], np.uint32), np.array([2], np.uint32)
    out = np.zeros(2, np.int64)
    assert hip.zgml_hip_resident_decode_batch(hip_backend.ctx, s1.handle, one.ctypes.data_as(u32p), zero.ctypes.data_as(u32p), cnt.ctypes.data_as(u32p), 2, out.ctypes.data) != 0
    assert "not a batched program" in hip_backend.last_error()
    hip.zgml_hip_clear_error(hip_backend.ctx)
    # nothing stuck: both programs still run
    assert sb.resident_decode_batch([1, 2], [0, 0], 3).shape == (B, 3)
    assert s1.resident_decode(1, 0, 3).shape == (3,)
    hip_backend.synchronize()
    assert not hip_backend.last_error(), hip_backend.last_error()
    s1.close(), m.close(), sb.close(), bm.close()
