"""GGUF Q3_K / Q2_K mat-vecs and matmuls on the MI355X against float64: the formats' cases of tests/sb_cases.py (shapes, pins, bound)."""
import pytest

from tests.sb_cases import matmul_against_float64, matmul_cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fmt,M,K,N,strided,pin", [(fmt, *c) for fmt in ("q3_k", "q2_k") for c in matmul_cases(fmt)])
def test_q23k_matmul_against_float64(hip_backend, fmt, M, K, N, strided, pin):
    matmul_against_float64(hip_backend, fmt, M, K, N, strided, pin)
