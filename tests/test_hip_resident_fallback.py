"""The device-resident loops against the bounds a batched plan assumed. The device patches the dynamic words itself, so each
loop probes the positions of its call on the host first and, when one leaves the plan's bounds, falls back to program order for
good — stepping has test_position_outside_the_compiled_bounds_falls_back_to_program_order for that; these are the resident
loops' own. Every program is compiled with its attentions' seq_kv at the smallest value a patch gives (1; T for a prefill chunk),
the tokens are compared with a second session stepping through the ordinary refresh, and the plan text shows the fall-back."""
import numpy as np
import pytest

from zgml_amd import llama
from tests.test_hip_batch_decode import launches, plan_text, stepped_tokens

pytestmark = pytest.mark.gpu


def n_launches(be, session):
    return len(launches(plan_text(be, session.handle)))


def fell_back(be, session, before, n_ops):
    assert not be.last_error(), be.last_error()
    after = n_launches(be, session)
    assert before < after <= n_ops, (before, after, n_ops)  # op by op now


def step_tokens(s, first, start, n):
    out, tok = [], first
    for pos in range(start, start + n):
        tok, _ = s.step(tok, pos, want_logits=False)
        out.append(tok)
    return out


@pytest.mark.parametrize("kv_quant_block", [0, 32])
def test_resident_decode_outside_the_compiled_bounds(hip_backend, kv_quant_block):
    """kv_quant_block = 32: the int8 KV cache, i.e. attention_kvq's bound instead of attention's"""
    cfg = llama.preset("tiny")
    cfg.kv_quant_block = kv_quant_block
    m = llama.Model(cfg)
    m.patch(0, 0)  # every seq_kv 1
    fns = llama.hip_backend_fns(hip_backend)
    s, s_ref = llama.Session(m, fns), llama.Session(m, fns)
    s.resident_setup(hip_backend)
    before = n_launches(hip_backend, s)
    got = s.resident_decode(3, 0, 6)
    fell_back(hip_backend, s, before, m.program.n_ops)
    assert got.tolist() == step_tokens(s_ref, 3, 0, 6)
    assert not hip_backend.last_error(), hip_backend.last_error()
    s.close(), s_ref.close(), m.close()


def test_resident_decode_batch_outside_the_compiled_bounds(hip_backend):
    B, first, start, counts = 3, [3, 40, 77], [0, 0, 0], [6, 3, 1]
    bm = llama.BatchModel(llama.preset("tiny"), B)
    bm.patch_batch([1] * B, [0] * B)
    fns = llama.hip_backend_fns(hip_backend)
    s, s_ref = llama.BatchSession(bm, fns, B), llama.BatchSession(bm, fns, B)
    s.resident_setup(hip_backend)
    before = n_launches(hip_backend, s)
    got = s.resident_decode_batch(first, start, counts)
    fell_back(hip_backend, s, before, bm.program.n_ops)
    assert got.tolist() == stepped_tokens(s_ref, first, start, counts).tolist()
    assert not hip_backend.last_error(), hip_backend.last_error()
    s.close(), s_ref.close(), bm.close()


def test_resident_prefill_outside_the_compiled_bounds(hip_backend):
    T, chunk = 4, [5, 9, 2, 7]
    m = llama.Model(llama.preset("tiny"), token_len=T)
    zeros = np.zeros(T, np.uint32)
    m.lib.zh_model_patch_tokens(m.ptr, zeros.ctypes.data, 0)  # every seq_kv T: the chunk at position 0
    fns = llama.hip_backend_fns(hip_backend)
    s, s_ref = llama.Session(m, fns), llama.Session(m, fns)
    s.resident_setup(hip_backend)
    before = n_launches(hip_backend, s)
    got = s.resident_prefill(chunk, T)  # positions T .. 2T - 1: seq_kv 2T
    fell_back(hip_backend, s, before, m.program.n_ops)
    want, _ = s_ref.prefill(chunk, T, want_logits=False)
    assert got == want
    assert not hip_backend.last_error(), hip_backend.last_error()
    s.close(), s_ref.close(), m.close()


def test_resident_decode_inside_the_compiled_bounds_keeps_the_plan(hip_backend):
    m = llama.Model(llama.preset("tiny"))  # as built: every seq_kv at max_seq_len
    fns = llama.hip_backend_fns(hip_backend)
    s, s_ref = llama.Session(m, fns), llama.Session(m, fns)
    s.resident_setup(hip_backend)
    before = n_launches(hip_backend, s)
    got = s.resident_decode(3, 0, 4)
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert n_launches(hip_backend, s) == before < m.program.n_ops
    assert got.tolist() == step_tokens(s_ref, 3, 0, 4)
    s.close(), s_ref.close(), m.close()
