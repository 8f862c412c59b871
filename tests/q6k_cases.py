"""GGUF Q6_K super-blocks in numpy (the format: zgml_amd/csrc/q6k.h): a block generator, the float64 dequantiser and the small
all-256 model config the Q4_K_M tests build."""
import numpy as np

BLOCK, BYTES = 256, 210


def q6k_blocks(rng, K, N, d=None, scale=None, ql_byte=None, qh_byte=None):
    """K * N / 256 random super-blocks, uint8 [n, 210]: d of both signs, every other byte uniform; a given value pins its field"""
    assert N % BLOCK == 0
    n = K * N // BLOCK
    raw = rng.integers(0, 256, (n, BYTES), dtype=np.uint8)
    dv = np.full(n, d) if d is not None else rng.choice(np.array([-1.0, 1.0]), n) * (1e-4 + rng.random(n) * 2e-3)
    raw[:, 208:210] = dv.astype(np.float16).view(np.uint8).reshape(n, 2)
    for lo, hi, v in [(192, 208, None if scale is None else scale & 255), (0, 128, ql_byte), (128, 192, qh_byte)]:
        if v is not None:
            raw[:, lo:hi] = v
    return raw


def q6k_weights(raw, K, N):
    """float64 [K, N]: w = d * scales[e / 16] * (q - 32), element e = 128 h + 32 g + l"""
    b = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1, BYTES)
    n = b.shape[0]
    ql = b[:, :128].reshape(n, 2, 2, 32)  # [h][g & 1][l]; the nibble is g >> 1
    low = np.stack([ql & 15, ql >> 4], axis=2).reshape(n, 2, 4, 32)
    qh = b[:, 128:192].reshape(n, 2, 32)
    high = np.stack([(qh >> (2 * g)) & 3 for g in range(4)], axis=2)
    q = (low | (high << 4)).reshape(n, BLOCK).astype(np.float64) - 32
    d = b[:, 208:210].copy().view(np.float16).astype(np.float64)
    sc = b[:, 192:208].copy().view(np.int8).astype(np.float64)
    return (np.repeat(d * sc, 16, axis=1) * q).reshape(K, N)


def model_config():
    """two layers, every projection width a multiple of 256, untied head: layer 0 all Q4_K; wv / w_down of layer 1 and the head Q6_K"""
    from zgml_amd import llama
    cfg = llama.preset("tiny")
    cfg.d_model, cfg.n_heads, cfg.n_kv_heads, cfg.d_ff, cfg.vocab_size, cfg.n_layers = 256, 4, 4, 512, 512, 2
    cfg.tied_lm_head = 0
    return cfg


# (K, N, block_size, data_len, accepted): 144 and 210 B per 256 elements; a byte too many; cols = 384; block 32 over 210-sized data
FORM_CASES = [(64, 256, 256, 64 * 144, True), (64, 256, 256, 64 * 210, True), (64, 256, 256, 64 * 210 + 1, False),
              (64, 384, 256, 96 * 210, False), (64, 256, 32, 64 * 210, False)]
Q6K_WEIGHTS = {7 + 2, 7 + 6, 14}  # weight order: per layer q, k, v, o, gate, up, down; then the head
