"""A Llama model in the Q5_K_M mix (llama.Q5_K_M_GGUF: Q5_K and Q6_K super-blocks) on the MI355X against the oracle running the same
values as f32 matmuls (llama.Q5_K_M_DENSE): greedy tokens equal, logits within 2e-4 of the logit range (as tests/test_hip_llama.py)."""
import numpy as np
import pytest

from zgml_amd import llama
from tests.q5k_cases import model_config

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("T", [1, 8])
def test_q5_k_m_model_matches_the_dense_oracle(hip_backend, oracle, T):
    cfg = model_config()  # T = 1: six decode steps; T = 8: two prefill chunks
    m_hip, m_ref = llama.Model(cfg, llama.Q5_K_M_GGUF, token_len=T), llama.Model(cfg, llama.Q5_K_M_DENSE, token_len=T)
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


def test_q5_k_m_resident_decode_equals_stepping(hip_backend):
    m = llama.Model(model_config(), llama.Q5_K_M_GGUF)
    s = llama.Session(m, llama.hip_backend_fns(hip_backend))
    s.resident_setup(hip_backend)
    got = s.resident_decode(5, 0, 16)
    want, _ = s.decode(5, 0, 16)
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert got.tolist() == want.tolist()
    s.close(), m.close()
