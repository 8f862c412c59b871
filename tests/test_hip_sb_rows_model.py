"""Models of GGUF super-block weights through the multi-row mat-vecs (ZGML_HIP_OPT_SMALL_M_MATVEC; sb_kernels.hip): batched decode of
three sequences against the oracle on the kind's dense twin (tokens equal, logits within 2e-4 of the logit range: the contract of
tests/test_hip_sb_model.py) and against the same model over the matrix-core kernels; every row of a four-token step against its single step."""
import numpy as np
import pytest

from zgml_amd import llama
from tests.sb_cases import model_config

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", [llama.Q4_K_M_GGUF, llama.IQ4_XS_GGUF])
def test_batched_decode_through_the_row_kernels(hip_backend, oracle, kind):
    cfg, B = model_config(), 3
    bm, bm_ref = llama.BatchModel(cfg, B, kind), llama.BatchModel(cfg, B, llama.DENSE_TWIN[kind])
    fns = llama.hip_backend_fns(hip_backend)
    s_rows, s_mm = llama.BatchSession(bm, fns, B, small_m_matvec=8), llama.BatchSession(bm, fns, B, small_m_matvec=False)
    s_ref = llama.BatchSession(bm_ref, oracle.backend_fns(), B)
    text = hip_backend.planText(s_rows.handle)
    assert "q6k-rows" in text and not any(t + "-matmul" in text for t in ("q4k", "q6k", "iq4xs")) and "-rows" not in hip_backend.planText(s_mm.handle)
    toks, pos = np.array([3, 11, 200]), np.array([0, 0, 0])
    for it in range(6):
        (t_rows, l_rows), (t_mm, _), (t_ref, l_ref) = [s.step(toks, pos) for s in (s_rows, s_mm, s_ref)]
        assert not hip_backend.last_error(), hip_backend.last_error()
        assert t_rows.tolist() == t_ref.tolist() == t_mm.tolist(), it
        assert (np.abs(l_rows - l_ref).max(axis=1) / np.abs(l_ref).max(axis=1) < 2e-4).all(), it
        toks, pos = t_ref, pos + 1
    for s in (s_rows, s_mm, s_ref):
        s.close()
    bm.close(), bm_ref.close()


def test_every_row_of_a_four_token_step_equals_its_single_step(hip_backend):
    """one sequence, four tokens per step (the verify plan: M = 4) under the option at 4: EVERY row's logits are the bytes of the
    T = 1 step over the same token at the same position"""
    cfg, toks = model_config(), [3, 11, 200, 7]
    m4, m1 = llama.BatchModel(cfg, 1, llama.Q4_K_M_GGUF, tokens_per_seq=4), llama.Model(cfg, llama.Q4_K_M_GGUF)
    fns = llama.hip_backend_fns(hip_backend)
    s4, s1 = llama.BatchSession(m4, fns, 1, small_m_matvec=4), llama.Session(m1, fns)
    assert "q4k-rows" in hip_backend.planText(s4.handle)
    t4, l4 = s4.step(toks, [0])
    for p, tok in enumerate(toks):
        t1, l1 = s1.step(tok, p)
        assert not hip_backend.last_error(), hip_backend.last_error()
        assert t4[p] == t1 and np.array_equal(l4[p], l1), p
    s4.close(), s1.close(), m4.close(), m1.close()
