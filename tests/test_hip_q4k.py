"""GGUF Q4_K mat-vecs and matmuls on the MI355X against float64: the format's cases of tests/sb_cases.py (shapes, pins, bound)."""
import pytest

from tests.sb_cases import matmul_against_float64, matmul_cases

pytestmark = pytest.mark.gpu

Q_BYTE = {None: None, "max": 0xFF, "mirror": 0x00}  # the case ids name Q4_K's two pins by their qs byte


@pytest.mark.parametrize("M,K,N,strided,q_byte", [(*c[:4], Q_BYTE[c[4]]) for c in matmul_cases("q4_k")])
def test_q4k_matmul_against_float64(hip_backend, M, K, N, strided, q_byte):
    matmul_against_float64(hip_backend, "q4_k", M, K, N, strided, {v: k for k, v in Q_BYTE.items()}[q_byte])
