"""Llama models in the Q3_K_M mix (Q3_K, Q4_K, Q5_K and Q6_K super-blocks at once) and the Q2_K mix (Q2_K, Q3_K, Q6_K) on the MI355X against
the oracle running the dense twins: greedy tokens equal, logits within 2e-4 of the logit range (tests/test_hip_q5k_model.py's bound); resident decode equals stepping."""
import numpy as np
import pytest

from zgml_amd import llama
from tests.q6k_cases import model_config

pytestmark = pytest.mark.gpu
KINDS = [llama.Q3_K_M_GGUF, llama.Q2_K_GGUF]  # the dense twin is the kind + 1


@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("kind", KINDS)
def test_q23k_model_matches_the_dense_oracle(hip_backend, oracle, kind, T):
    cfg = model_config()  # T = 1: six decode steps, then resident decode against stepping; T = 8: two prefill chunks
    m_hip, m_ref = llama.Model(cfg, kind, token_len=T), llama.Model(cfg, kind + 1, token_len=T)
    s_hip, s_ref = llama.Session(m_hip, llama.hip_backend_fns(hip_backend)), llama.Session(m_ref, oracle.backend_fns())
    tok = 3
    for it in range(6 if T == 1 else 2):
        toks = [(7 * i + 3 + it) % cfg.vocab_size for i in range(T)]
        (t_hip, l_hip), (t_ref, l_ref) = [s.step(tok, it) if T == 1 else s.prefill(toks, it * T) for s in (s_hip, s_ref)]
        assert not hip_backend.last_error(), hip_backend.last_error()
        assert t_hip == t_ref, (it, t_hip, t_ref)
        assert np.abs(l_hip - l_ref).max() / np.abs(l_ref).max() < 2e-4, it
        tok = t_ref
    if T == 1:  # and the resident loop decodes the 16 tokens that stepping does
        s_hip.resident_setup(hip_backend)
        assert s_hip.resident_decode(5, 0, 16).tolist() == s_hip.decode(5, 0, 16)[0].tolist() and not hip_backend.last_error()
    s_hip.close(), s_ref.close(), m_hip.close(), m_ref.close()

