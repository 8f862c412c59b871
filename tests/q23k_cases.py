"""GGUF Q3_K and Q2_K super-blocks in numpy, written from the formats' public definition (256 flat elements per block; element e):
  Q3_K, 110 B: hmask[32] | qs[64] | scales[12] | f16 d.   low = (qs[32 (e >> 7) + (e & 31)] >> 2 ((e >> 5) & 3)) & 3,
    high = (hmask[e & 31] >> (e >> 5)) & 1, q = low + 4 high - 4; sub-block s = e >> 4 has the 6-bit scale
    (scales[s] & 15 if s < 8 else scales[s - 8] >> 4) | ((scales[8 + (s & 3)] >> 2 (s >> 2)) & 3) << 4;   w = d (sc - 32) q
  Q2_K, 84 B: scales[16] | qs[64] | f16 d | f16 dmin.   q = the low rule above;   w = d (scales[s] & 15) q - dmin (scales[s] >> 4)
A block generator (a given value pins a field) and the float64 dequantisers."""
import numpy as np

BYTES = {"q3_k": 110, "q2_k": 84}
HALVES = {"q3_k": {"d": (108, 1e-4, 2e-3)}, "q2_k": {"d": (80, 1e-4, 2e-3), "dmin": (82, 1e-3, 2e-2)}}  # f16 fields: (offset, least, largest magnitude)
FIELDS = {"q3_k": {"hmask": (0, 32), "qs": (32, 96), "scales_lo": (96, 104), "scales_hi": (104, 108)}, "q2_k": {"scales": (0, 16), "qs": (16, 80)}}  # byte fields: (from, to)
E = np.arange(256)
QS_AT, QS_SHIFT = 32 * (E >> 7) + (E & 31), 2 * ((E >> 5) & 3)


def blocks(fmt, rng, K, N, **pin):
    """K * N / 256 random super-blocks, uint8 [n, BYTES]: d (dmin) of both signs, every other byte uniform; pin: field = value"""
    n = K * N // 256
    raw = rng.integers(0, 256, (n, BYTES[fmt]), dtype=np.uint8)
    for name, (off, lo, hi) in HALVES[fmt].items():
        h = np.full(n, pin[name]) if name in pin else rng.choice(np.array([-1.0, 1.0]), n) * (lo + rng.random(n) * (hi - lo))
        raw[:, off:off + 2] = h.astype(np.float16).view(np.uint8).reshape(n, 2)
    for name, (a, b) in FIELDS[fmt].items():
        if name in pin:
            raw[:, a:b] = pin[name]
    return raw


def _f16(b, off):
    return b[:, off:off + 2].copy().view(np.float16).astype(np.float64)


def q3k_weights(raw, K, N):
    r = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1, 110)
    b = r.astype(np.int64)
    q = ((b[:, 32:96][:, QS_AT] >> QS_SHIFT) & 3) + 4 * ((b[:, :32][:, E & 31] >> (E >> 5)) & 1) - 4
    s, sc = np.arange(16), b[:, 96:108]
    six = np.where(s < 8, sc[:, s % 8] & 15, sc[:, s % 8] >> 4) | (((sc[:, 8 + (s & 3)] >> (2 * (s >> 2))) & 3) << 4)
    return (_f16(r, 108) * np.repeat(six - 32, 16, axis=1) * q).reshape(K, N)


def q2k_parts(raw, K, N):  # the pair (d sc q, dmin m): the weight is their difference, and the kernels sum the two apart
    r = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1, 84)
    b = r.astype(np.int64)
    q = (b[:, 16:80][:, QS_AT] >> QS_SHIFT) & 3
    return (_f16(r, 80) * np.repeat(b[:, :16] & 15, 16, axis=1) * q).reshape(K, N), (_f16(r, 82) * np.repeat(b[:, :16] >> 4, 16, axis=1)).reshape(K, N)


def parts(fmt, raw, K, N):  # (a, b) with w = a - b for either format (Q3_K: b = 0)
    return q2k_parts(raw, K, N) if fmt == "q2_k" else (q3k_weights(raw, K, N), np.zeros((K, N)))


# (K, N, block_size, data_len, accepted): the exact byte count; a byte too many; cols = 384; blocks of 32 over super-block-sized data
FORM_CASES = {f: [(64, 256, 256, 64 * B, True), (64, 256, 256, 64 * B + 1, False), (64, 384, 256, 96 * B, False), (64, 256, 32, 64 * B, False)] for f, B in BYTES.items()}
