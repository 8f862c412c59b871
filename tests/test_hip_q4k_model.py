"""A Llama model of GGUF Q4_K projections (llama.Q4_K_GGUF) on the MI355X against the oracle running the same values as f32 matmuls
(llama.Q4_K_DENSE): greedy tokens equal, logits within 2e-4 of the logit range (the contract of tests/test_hip_llama.py)."""
import numpy as np
import pytest

from zgml_amd import llama

pytestmark = pytest.mark.gpu


def config():
    """every projection width a multiple of 256, so every projection (and the untied LM head) is Q4_K"""
    cfg = llama.preset("tiny")
    cfg.d_model, cfg.n_heads, cfg.n_kv_heads, cfg.d_ff, cfg.vocab_size, cfg.n_layers = 256, 4, 4, 512, 512, 2
    cfg.tied_lm_head = 0
    return cfg


@pytest.mark.parametrize("T", [1, 8])
def test_q4k_model_matches_the_dense_oracle(hip_backend, oracle, T):
    """T = 1: six decode steps; T = 8: two prefill chunks"""
    cfg = config()
    m_hip, m_ref = llama.Model(cfg, llama.Q4_K_GGUF, token_len=T), llama.Model(cfg, llama.Q4_K_DENSE, token_len=T)
    assert all(m_hip.program.qweights[i].block_size == 256 for i in range(m_hip.program.n_qweights))
    s_hip, s_ref = llama.Session(m_hip, llama.hip_backend_fns(hip_backend)), llama.Session(m_ref, oracle.backend_fns())
    tok = 3
    for it in range(6 if T == 1 else 2):
        if T == 1:
            (t_hip, l_hip), (t_ref, l_ref) = s_hip.step(tok, it), s_ref.step(tok, it)
        else:
            toks = [(7 * i + 3 + it) % cfg.vocab_size for i in range(T)]
            (t_hip, l_hip), (t_ref, l_ref) = s_hip.prefill(toks, it * T), s_ref.prefill(toks, it * T)
        assert not hip_backend.last_error(), hip_backend.last_error()
        assert t_hip == t_ref, (it, t_hip, t_ref)
        assert np.abs(l_hip - l_ref).max() / np.abs(l_ref).max() < 2e-4, it
        tok = t_ref
    s_hip.close(), s_ref.close(), m_hip.close(), m_ref.close()


def test_q4k_resident_decode_equals_stepping(hip_backend):
    m = llama.Model(config(), llama.Q4_K_GGUF)
    s = llama.Session(m, llama.hip_backend_fns(hip_backend))
    s.resident_setup(hip_backend)
    got = s.resident_decode(5, 0, 16)
    want, _ = s.decode(5, 0, 16)
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert got.tolist() == want.tolist()
    s.close(), m.close()
