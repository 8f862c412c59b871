"""GGUF Q5_K super-blocks in numpy (the format: zgml_amd/csrc/q5k.h): a block generator, the float64 dequantiser in its two parts
and the small all-256 model config the Q5_K_M tests build."""
import numpy as np

from tests.q4k_cases import q4k_blocks, q4k_parts
from tests.q6k_cases import Q6K_WEIGHTS, model_config  # noqa: F401  (the mix's layout rule is Q4_K_M's)

BLOCK, BYTES = 256, 176


def q5k_blocks(rng, K, N, d=None, dmin=None, scale_byte=None, ql_byte=None, qh_byte=None):
    """K * N / 256 random super-blocks, uint8 [n, 176]: q4k_blocks (header, then the 128 nibble bytes) with the 32 qh bytes between"""
    b4 = q4k_blocks(rng, K, N, d=d, dmin=dmin, scale_byte=scale_byte, q_byte=ql_byte)
    qh = rng.integers(0, 256, (b4.shape[0], 32), dtype=np.uint8) if qh_byte is None else np.full((b4.shape[0], 32), qh_byte, np.uint8)
    return np.concatenate([b4[:, :16], qh, b4[:, 16:]], axis=1)


def q5k_parts(raw, K, N):
    """float64 [K, N] pair (d * sc * q, dmin * m), q = nibble | high bit << 4 with element 32 j + l taking bit j of qh[l]"""
    b = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1, BYTES)
    a4, m = q4k_parts(np.concatenate([b[:, :16], b[:, 48:]], axis=1), K, N)  # d * sc * nibble
    one, _ = q4k_parts(np.concatenate([b[:, :16], np.full((b.shape[0], 128), 0x11, np.uint8)], axis=1), K, N)  # d * sc
    high = np.stack([(b[:, 16:48] >> j) & 1 for j in range(8)], axis=1).reshape(K, N).astype(np.float64)
    return a4 + 16.0 * one * high, m


# (K, N, block_size, data_len, accepted): 176 B per 256 elements; a byte too many; cols = 384; 512 blocks of 32 need 9216 or 17408 B
FORM_CASES = [(64, 256, 256, 64 * 176, True), (64, 256, 256, 64 * 176 + 1, False), (64, 384, 256, 96 * 176, False), (64, 256, 32, 64 * 176, False)]
