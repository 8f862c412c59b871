"""GGUF Q4_K super-blocks in numpy (the format: zgml_amd/csrc/q4k.h): a block generator and the float64 dequantiser."""
import numpy as np

BLOCK, BYTES = 256, 144


def q4k_blocks(rng, K, N, d=None, dmin=None, scale_byte=None, q_byte=None):
    """K * N / 256 random super-blocks, uint8 [n, 144]: d, dmin of both signs, every other byte uniform; a given value pins its field"""
    assert N % BLOCK == 0
    n = K * N // BLOCK
    raw = rng.integers(0, 256, (n, BYTES), dtype=np.uint8)
    sign = lambda: rng.choice(np.array([-1.0, 1.0]), n)
    half = lambda v, lo, hi: (np.full(n, v) if v is not None else sign() * (lo + rng.random(n) * (hi - lo))).astype(np.float16)
    raw[:, 0:2] = half(d, 1e-4, 2e-3).view(np.uint8).reshape(n, 2)
    raw[:, 2:4] = half(dmin, 1e-3, 2e-2).view(np.uint8).reshape(n, 2)
    if scale_byte is not None:
        raw[:, 4:16] = scale_byte
    if q_byte is not None:
        raw[:, 16:] = q_byte
    return raw


def q4k_parts(raw, K, N):
    """float64 [K, N] pair (d * sc * q, dmin * m): the weight is their difference, and the kernels sum the two apart"""
    b = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1, BYTES)
    n = b.shape[0]
    d = b[:, 0:2].copy().view(np.float16).astype(np.float64)
    dmin = b[:, 2:4].copy().view(np.float16).astype(np.float64)
    s = b[:, 4:16].astype(np.int64)
    sc, m = np.empty((n, 8)), np.empty((n, 8))
    for j in range(8):
        if j < 4:
            sc[:, j], m[:, j] = s[:, j] & 63, s[:, j + 4] & 63
        else:
            sc[:, j] = (s[:, j + 4] & 15) | ((s[:, j - 4] >> 6) << 4)
            m[:, j] = (s[:, j + 4] >> 4) | ((s[:, j] >> 6) << 4)
    qs = b[:, 16:].reshape(n, 4, 32)
    q = np.stack([qs & 15, qs >> 4], axis=2).reshape(n, BLOCK).astype(np.float64)  # element 64 i + 32 h + l
    return (np.repeat(d * sc, 32, axis=1) * q).reshape(K, N), np.repeat(dmin * m, 32, axis=1).reshape(K, N)
