"""GGUF IQ4_XS in numpy, written from the format's public definition, with its block generator and pins. 136 B per 256 flat elements:
f16 d | u16 scales_h | scales_l[4] | qs[128]. Sub-block ib = e >> 5, j = e & 31: ls = ((scales_l[ib >> 1] >> 4 (ib & 1)) & 15) |
((scales_h >> 2 ib) & 3) << 4; idx = the low (j < 16) or high nibble of qs[16 ib + (j & 15)]; w = d (ls - 32) KVALUES[idx]."""
import numpy as np

from tests.sb_cases import F16_MAX

KVALUES = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], np.float64)
IB = np.arange(8)


def iq4xs_parts(raw, K, N):
    """float64 (a, zeros) [K, N]: w = a, no min term"""
    r = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1, 136)
    b, d = r.astype(np.int64), r[:, 0:2].copy().view(np.float16).astype(np.float64)
    ls = ((b[:, 4 + (IB >> 1)] >> (4 * (IB & 1))) & 15) | ((((b[:, 2:3] | b[:, 3:4] << 8) >> (2 * IB)) & 3) << 4)
    qs = b[:, 8:].reshape(-1, 8, 16)
    kv = KVALUES[np.concatenate([qs & 15, qs >> 4], axis=2)]  # [block, ib, j]
    return (d[:, :, None] * (ls - 32)[:, :, None] * kv).reshape(K, N), np.zeros((K, N))


def iq4xs_blocks(rng, K, N, **pin):
    """K * N / 256 random blocks, uint8 [n, 136]: d of both signs in [1e-4, 2e-3], every other byte uniform; pin: field = value"""
    n = K * N // 256
    raw = rng.integers(0, 256, (n, 136), dtype=np.uint8)
    d = np.full(n, pin["d"]) if "d" in pin else rng.choice(np.array([-1.0, 1.0]), n) * (1e-4 + rng.random(n) * (2e-3 - 1e-4))
    raw[:, 0:2] = d.astype(np.float16).view(np.uint8).reshape(n, 2)
    for name, (a, b) in (("scales_h", (2, 4)), ("scales_l", (4, 8)), ("qs", (8, 136))):
        if name in pin:
            raw[:, a:b] = np.array([pin[name]], "<u2").view(np.uint8) if name == "scales_h" else pin[name]
    return raw


# the largest finite weights (ls = 0, index 0: -32 * -127 = 4064); ls = 32 everywhere; index 0 in columns 0..15 of every item and 15 in
# columns 16..31: both ends of the table and the nibble-to-column order
PINS = {"max": dict(d=F16_MAX, scales_h=0, scales_l=0, qs=0), "zero": dict(scales_l=0, scales_h=0xAAAA), "table ends": dict(qs=0xF0)}
