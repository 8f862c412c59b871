"""GGUF Q5_K mat-vecs and matmuls on the MI355X against float64: the format's cases of tests/sb_cases.py (shapes, pins, bound)."""
import pytest

from tests.sb_cases import matmul_against_float64, matmul_cases

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("M,K,N,strided,pin", matmul_cases("q5_k"))
def test_q5k_matmul_against_float64(hip_backend, M, K, N, strided, pin):
    matmul_against_float64(hip_backend, "q5_k", M, K, N, strided, pin)
