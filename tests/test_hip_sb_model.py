"""Llama models of GGUF super-block projections (the gguf kinds of tests/sb_cases.py's MIXES: Q4_K alone, the Q4_K_M, Q5_K_M and Q3_K_M
mixes, the Q2_K mix) on the MI355X against the oracle running the same values as f32 matmuls (the kind's dense twin): greedy tokens
equal, logits within 2e-4 of the logit range (the contract of tests/test_hip_llama.py); resident decode equals stepping."""
import numpy as np
import pytest

from zgml_amd import llama
from tests.sb_cases import MIXES, model_config

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("kind", list(MIXES))
def test_model_matches_the_dense_oracle(hip_backend, oracle, kind, T):
    """T = 1: six decode steps; T = 8: two prefill chunks"""
    cfg = model_config()
    m_hip, m_ref = llama.Model(cfg, kind, token_len=T), llama.Model(cfg, llama.DENSE_TWIN[kind], token_len=T)
    qws = [m_hip.program.qweights[i] for i in range(m_hip.program.n_qweights)]
    assert all(q.block_size == 256 for q in qws) and [q.data_len * 256 // (q.rows * q.cols) for q in qws] == MIXES[kind]
    s_hip, s_ref = llama.Session(m_hip, llama.hip_backend_fns(hip_backend)), llama.Session(m_ref, oracle.backend_fns())
    tok = 3
    for it in range(6 if T == 1 else 2):
        toks = [(7 * i + 3 + it) % cfg.vocab_size for i in range(T)]
        (t_hip, l_hip), (t_ref, l_ref) = [s.step(tok, it) if T == 1 else s.prefill(toks, it * T) for s in (s_hip, s_ref)]
        assert not hip_backend.last_error(), hip_backend.last_error()
        assert t_hip == t_ref, (it, t_hip, t_ref)
        assert np.abs(l_hip - l_ref).max() / np.abs(l_ref).max() < 2e-4, it
        tok = t_ref
    s_hip.close(), s_ref.close(), m_hip.close(), m_ref.close()


@pytest.mark.parametrize("kind", list(MIXES))
def test_resident_decode_equals_stepping(hip_backend, kind):
    m = llama.Model(model_config(), kind)
    s = llama.Session(m, llama.hip_backend_fns(hip_backend))
    s.resident_setup(hip_backend)
    got = s.resident_decode(5, 0, 16)
    want, _ = s.decode(5, 0, 16)
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert got.tolist() == want.tolist()
    s.close(), m.close()
