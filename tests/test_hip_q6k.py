"""GGUF Q6_K mat-vecs and matmuls on the MI355X against float64: the format's cases of tests/sb_cases.py (shapes, pins, bound)."""
import pytest

from tests.sb_cases import matmul_against_float64, matmul_cases

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("M,K,N,strided,pin", matmul_cases("q6_k"))
def test_q6k_matmul_against_float64(hip_backend, M, K, N, strided, pin):
    matmul_against_float64(hip_backend, "q6_k", M, K, N, strided, pin)
