"""The GGUF super-block formats (Q2_K .. Q6_K: 256 flat elements per block; element e) in numpy, written from the formats' public
definitions, as one table keyed by the upload name. What a test of the family needs beyond it is stated here once as well: a block
generator (a given value pins a field), the float64 dequantisers as the pair (a, b) with w = a - b (the kernels sum the two apart),
the bound, the program helpers and the small all-256 model with its mixes.
  Q2_K, 84 B: scales[16] | qs[64] | f16 d | f16 dmin.   q = (qs[32 (e >> 7) + (e & 31)] >> 2 ((e >> 5) & 3)) & 3; sub-block s = e >> 4:
    w = d (scales[s] & 15) q - dmin (scales[s] >> 4)
  Q3_K, 110 B: hmask[32] | qs[64] | scales[12] | f16 d.   low = Q2_K's q, high = (hmask[e & 31] >> (e >> 5)) & 1, q = low + 4 high - 4;
    sc = (scales[s] & 15 if s < 8 else scales[s - 8] >> 4) | ((scales[8 + (s & 3)] >> 2 (s >> 2)) & 3) << 4;   w = d (sc - 32) q
  Q4_K, 144 B: f16 d | f16 dmin | scales[12] | qs[128].   sub-block j = e >> 5; j < 4: sc = scales[j] & 63, m = scales[j + 4] & 63; else
    sc = scales[j + 4] & 15 | scales[j - 4] >> 6 << 4, m = scales[j + 4] >> 4 | scales[j] >> 6 << 4; q = the low (j even) or high
    nibble of qs[32 (j >> 1) + (e & 31)];   w = d sc q - dmin m
  Q5_K, 176 B: Q4_K's header | qh[32] | qs[128].   q = Q4_K's nibble | ((qh[e & 31] >> j) & 1) << 4;   w = d sc q - dmin m
  Q6_K, 210 B: ql[128] | qh[64] | int8 scales[16] | f16 d.   h = e >> 7, g = (e >> 5) & 3, l = e & 31: q = the low (g < 2) or high nibble
    of ql[64 h + 32 (g & 1) + l] | ((qh[32 h + l] >> 2 g) & 3) << 4;   w = d scales[e >> 4] (q - 32)"""
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

from zgml_amd import DeviceOp, DeviceProgram, ProgramIO, QuantizedWeightUpload, llama

f32, f64 = np.float32, np.float64
F16_MAX = 65504.0  # |w| <= 63 * 32 d (Q5_K, the widest): every f16 keeps the f32 sums of the tests' shapes finite
E = np.arange(256)
QS_AT, QS_SHIFT = 32 * (E >> 7) + (E & 31), 2 * ((E >> 5) & 3)  # the 2-bit planes: byte and shift of element e


def _f16(b, off):
    return b[:, off:off + 2].copy().view(np.float16).astype(f64)


def _blocks(raw, nbytes):
    r = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1, nbytes)
    return r, r.astype(np.int64)


def q2k_parts(raw, K, N):
    r, b = _blocks(raw, 84)
    q = (b[:, 16:80][:, QS_AT] >> QS_SHIFT) & 3
    return (_f16(r, 80) * np.repeat(b[:, :16] & 15, 16, axis=1) * q).reshape(K, N), (_f16(r, 82) * np.repeat(b[:, :16] >> 4, 16, axis=1)).reshape(K, N)


def q3k_parts(raw, K, N):
    r, b = _blocks(raw, 110)
    q = ((b[:, 32:96][:, QS_AT] >> QS_SHIFT) & 3) + 4 * ((b[:, :32][:, E & 31] >> (E >> 5)) & 1) - 4
    s, sc = np.arange(16), b[:, 96:108]
    six = np.where(s < 8, sc[:, s % 8] & 15, sc[:, s % 8] >> 4) | (((sc[:, 8 + (s & 3)] >> (2 * (s >> 2))) & 3) << 4)
    return (_f16(r, 108) * np.repeat(six - 32, 16, axis=1) * q).reshape(K, N), np.zeros((K, N))


def q4k_parts(raw, K, N):
    r, s = _blocks(raw, 144)
    n, s = len(r), s[:, 4:16]
    sc, m = np.empty((n, 8)), np.empty((n, 8))
    for j in range(8):
        if j < 4:
            sc[:, j], m[:, j] = s[:, j] & 63, s[:, j + 4] & 63
        else:
            sc[:, j] = (s[:, j + 4] & 15) | ((s[:, j - 4] >> 6) << 4)
            m[:, j] = (s[:, j + 4] >> 4) | ((s[:, j] >> 6) << 4)
    qs = r[:, 16:].reshape(n, 4, 32)
    q = np.stack([qs & 15, qs >> 4], axis=2).reshape(n, 256).astype(f64)  # element 64 i + 32 h + l
    return (np.repeat(_f16(r, 0) * sc, 32, axis=1) * q).reshape(K, N), np.repeat(_f16(r, 2) * m, 32, axis=1).reshape(K, N)


def q5k_parts(raw, K, N):
    r, _ = _blocks(raw, 176)
    a4, m = q4k_parts(np.concatenate([r[:, :16], r[:, 48:]], axis=1), K, N)  # d * sc * nibble
    one, _ = q4k_parts(q4k_ones(r), K, N)  # d * sc
    high = np.stack([(r[:, 16:48] >> j) & 1 for j in range(8)], axis=1).reshape(K, N).astype(f64)  # element 32 j + l: bit j of qh[l]
    return a4 + 16.0 * one * high, m


def q6k_parts(raw, K, N):
    r, _ = _blocks(raw, 210)
    n = len(r)
    ql = r[:, :128].reshape(n, 2, 2, 32)  # [h][g & 1][l]; the nibble is g >> 1
    low = np.stack([ql & 15, ql >> 4], axis=2).reshape(n, 2, 4, 32)
    qh = r[:, 128:192].reshape(n, 2, 32)
    high = np.stack([(qh >> (2 * g)) & 3 for g in range(4)], axis=2)
    q = (low | (high << 4)).reshape(n, 256).astype(f64) - 32
    sc = r[:, 192:208].copy().view(np.int8).astype(f64)
    return (np.repeat(_f16(r, 208) * sc, 16, axis=1) * q).reshape(K, N), np.zeros((K, N))


def q4k_ones(raw):
    """the 16-byte headers of Q4_K / Q5_K blocks over Q4_K nibbles of 1: q4k_parts gives (d * sc, dmin * m)"""
    return np.concatenate([raw[:, :16], np.full((len(raw), 128), 0x11, np.uint8)], axis=1)


@dataclass
class Format:
    nbytes: int
    halves: dict            # f16 fields, in draw order: name -> (offset, least, largest magnitude)
    fields: dict            # byte fields: name -> (from, to)
    parts: Callable         # (raw, K, N) -> float64 [K, N] pair (a, b), w = a - b
    has_min: bool           # b is the format's min term (else zeros)
    hashed: list            # (from, to, mask): bytes the host model builder hashes, so they take every value of the mask
    drawn_last: Optional[str] = None  # a byte field the generator draws after everything else (Q5_K's bytes were Q4_K's, then qh)


FORMATS = {
    "q2_k": Format(84, {"d": (80, 1e-4, 2e-3), "dmin": (82, 1e-3, 2e-2)}, {"scales": (0, 16), "qs": (16, 80)}, q2k_parts, True, [(16, 32, 255)]),
    "q3_k": Format(110, {"d": (108, 1e-4, 2e-3)}, {"hmask": (0, 32), "qs": (32, 96), "scales_lo": (96, 104), "scales_hi": (104, 108)}, q3k_parts, False,
                   [(16, 32, 255)]),
    "q4_k": Format(144, {"d": (0, 1e-4, 2e-3), "dmin": (2, 1e-3, 2e-2)}, {"scales": (4, 16), "qs": (16, 144)}, q4k_parts, True, [(16, 32, 255), (4, 16, 63)]),
    "q5_k": Format(176, {"d": (0, 1e-4, 2e-3), "dmin": (2, 1e-3, 2e-2)}, {"scales": (4, 16), "qh": (16, 48), "qs": (48, 176)}, q5k_parts, True, [(16, 32, 255)],
                   drawn_last="qh"),
    "q6_k": Format(210, {"d": (208, 1e-4, 2.1e-3)}, {"ql": (0, 128), "qh": (128, 192), "scales": (192, 208)}, q6k_parts, False,
                   [(16, 32, 255), (192, 208, 255)]),
}


def blocks(fmt, rng, K, N, **pin):
    """K * N / 256 random super-blocks, uint8 [n, nbytes]: d (dmin) of both signs, every other byte uniform; pin: field = value"""
    f = FORMATS[fmt]
    assert N % 256 == 0 and set(pin) <= set(f.halves) | set(f.fields), pin
    n = K * N // 256
    lo, hi = f.fields[f.drawn_last] if f.drawn_last else (0, 0)
    raw = rng.integers(0, 256, (n, f.nbytes - (hi - lo)), dtype=np.uint8)
    for name, (off, least, largest) in f.halves.items():
        h = np.full(n, pin[name]) if name in pin else rng.choice(np.array([-1.0, 1.0]), n) * (least + rng.random(n) * (largest - least))
        raw[:, off:off + 2] = h.astype(np.float16).view(np.uint8).reshape(n, 2)
    if hi > lo:
        last = np.zeros((n, hi - lo), np.uint8) if f.drawn_last in pin else rng.integers(0, 256, (n, hi - lo), dtype=np.uint8)
        raw = np.concatenate([raw[:, :lo], last, raw[:, lo:]], axis=1)
    for name, (a, b) in f.fields.items():
        if name in pin:
            raw[:, a:b] = pin[name]
    return raw


def parts(fmt, raw, K, N):
    return FORMATS[fmt].parts(raw, K, N)


# (K, N, block_size, data_len, accepted) per format: the exact byte count; a byte too many; cols = 384; blocks of 32 over super-block-
# sized data (Q4_K's 144 B per 256 are Q4_0's 18 B per 32: the block size tells the two apart; 64 is neither); Q4_K's bytes as "q6_k"
FORM_CASES = {f: [(64, 256, 256, 64 * B, True), (64, 256, 256, 64 * B + 1, False), (64, 384, 256, 96 * B, False), (64, 256, 32, 64 * B, f == "q4_k")]
              for f, B in ((f, row.nbytes) for f, row in FORMATS.items())}
FORM_CASES["q4_k"].append((64, 256, 64, 64 * 144, False))
FORM_CASES["q6_k"].insert(0, (64, 256, 256, 64 * 144, True))


def run(be, prog, outs):
    """compile, one execute per entry of outs ([(buffer, elements)]), free: the buffers read back, per execute"""
    h = be.compileProgram(prog)
    assert h, be.last_error()
    try:
        res = []
        for o in outs:
            bufs = [np.zeros(n, f32) for _, n in o]
            be.executeProgram(h, [], [ProgramIO(i, b) for (i, _), b in zip(o, bufs)])
            res.append(bufs)
    finally:
        be.freeProgram(h)
    assert not be.last_error(), be.last_error()
    return res


def check(got, x, a, b):
    """per output |y - x @ (a - b)| <= 2e-5 * sum_k |x[k]| * (|a| + |b|) + 1e-30: the project's mat-vec bound, its magnitude over BOTH
    terms (the kernels sum them apart, and they cancel in w); zero where a and b are"""
    x = x.astype(f64)
    assert np.all(np.abs(got - x @ (a - b)) <= 2e-5 * (np.abs(x) @ (np.abs(a) + np.abs(b))) + 1e-30)


def qmatmul(be, qw, x, M, K, N, strided=False):
    """x [M, K] through one qmatmul over the upload qw, rows dense or (strided) at offsets and row strides of their own: y [M, N]"""
    in_off, in_rs, dst_off, dst_rs = (3, K + 5, 7, N + 9) if strided else (0, K, 0, N)
    xin, ys = np.zeros(in_off + M * in_rs, f32), dst_off + M * dst_rs
    for m in range(M):
        xin[in_off + m * in_rs:][:K] = x[m]
    prog = DeviceProgram(ops=[DeviceOp.qmatmul(1, 0, 0, M, N, K, in_off, in_rs if strided else 0, dst_off, dst_rs if strided else 0)],
                         buffer_sizes=[xin.size, ys], initial_uploads=[ProgramIO(0, xin)], qweights=[qw])
    y = run(be, prog, [[(1, ys)]])[0][0]
    return np.stack([y[dst_off + m * dst_rs:][:N] for m in range(M)])


# The largest finite weights (every bit set, d the largest f16, dmin = -d; Q6_K: q = 0 under the scale -128); every factor zero (Q3_K:
# every 6-bit scale 32; Q6_K: q = 32). Q4_K: max's mirror q = 0. Q5_K: q = 16 everywhere (the high plane alone). Q3_K: q = 4 - 4
# everywhere; the low plane alone (q = low - 4). Q2_K: the min term alone.
PINS = {"q4_k": {"max": dict(d=F16_MAX, dmin=-F16_MAX, scales=0xFF, qs=0xFF), "mirror": dict(d=F16_MAX, dmin=-F16_MAX, scales=0xFF, qs=0x00)},
        "q5_k": {"max": dict(d=F16_MAX, dmin=-F16_MAX, scales=0xFF, qs=0xFF, qh=0xFF), "high only": dict(qs=0, qh=0xFF), "zero": dict(scales=0)},
        "q6_k": {"max": dict(d=F16_MAX, scales=0x80, ql=0, qh=0), "zero": dict(ql=0, qh=0xAA)},
        "q3_k": {"max": dict(d=-F16_MAX, hmask=0xFF, qs=0xFF, scales_lo=0xFF, scales_hi=0xFF), "zero": dict(scales_lo=0, scales_hi=0xAA),
                 "q zero": dict(qs=0, hmask=0xFF), "low only": dict(hmask=0)},
        "q2_k": {"max": dict(d=F16_MAX, dmin=-F16_MAX, scales=0xFF, qs=0xFF), "zero": dict(scales=0), "min only": dict(qs=0)}}
# M = 1 (kSbRound = 256 k, kSbSweep = 64, kSbRoundMaxParts = 16): one column block and one k; K odd, below a sweep; K one past a one-round
# share (two parts, the last of one k); 16 rounds over two column blocks (16 parts of one round: the cap); three column blocks, K no
# multiple of the sweep; K one past 16 rounds (the cap makes parts of two rounds). M > 1 (row tile 16, two per workgroup over M = 16;
# chunk 64 k dealt to 8 waves): K of 1.5 chunks; K no multiple of 8 over two column blocks (16 chunks: two per wave); strides and
# offsets. Q4_K keeps shapes of its own: its split edges come from kSb4ShareMinSweeps (K = 261: one past the 256-k share of a part,
# with a ragged last part), and it has no cap to pass.
SHAPES = [(1, K, N, False) for K, N in [(1, 256), (37, 256), (257, 256), (4096, 512), (577, 768), (4097, 256)]] + \
         [(M, K, N, False) for K, N in [(96, 256), (1001, 512)] for M in (2, 5, 16, 17, 33)] + [(5, 1000, 512, True)]
SHAPES_Q4K = [(1, K, N, False) for K, N in [(1, 256), (37, 256), (261, 256), (4096, 512), (577, 768)]] + \
             [(M, K, N, False) for K, N in [(96, 256), (1000, 512)] for M in (2, 5, 16, 17, 33)] + [(5, 1000, 512, True)]


def matmul_cases(fmt):
    """(M, K, N, strided, pin) of a format: its shapes unpinned, then every pin at M = 1 and 5"""
    return [(*shape, None) for shape in (SHAPES_Q4K if fmt == "q4_k" else SHAPES)] + [(M, 96, 256, False, pin) for M in (1, 5) for pin in PINS[fmt]]


def pinned_values_hold(fmt, pin, raw, a, b, got):
    """the exact values a pin is there to produce"""
    if pin == "max":
        a_max, b_min = {"q4_k": (63 * 15, -63), "q5_k": (63 * 31, -63), "q6_k": (128 * 32, 0), "q3_k": (-93, 0), "q2_k": (45, -15)}[fmt]
        assert a.min() == a.max() == a_max * F16_MAX and b.min() == b.max() == b_min * F16_MAX
    elif pin == "mirror":
        assert a.max() == 0 and b.min() == b.max() == -63 * F16_MAX
    elif pin in ("zero", "q zero"):
        assert not a.any() and not b.any() and not got.any()
    elif pin == "high only":  # 16 times the Q4_K block of the same headers over nibbles of 1: d * sc
        assert a.any() and np.array_equal(a, 16 * parts("q4_k", q4k_ones(raw), *a.shape)[0])
    elif pin == "low only":  # q = low - 4 < 0
        assert a.any() and not raw[:, :32].any() and (np.sign(a[:, :16]) == np.sign(a[:, :1])).all()
    elif pin == "min only":
        assert not a.any() and got.any() and (b[:, :16] != b[:, 16:32]).any()


def matmul_against_float64(be, fmt, M, K, N, strided, pin):
    """the body of the formats' test_*_matmul_against_float64: seeded blocks and x through one qmatmul, against float64"""
    rng = np.random.default_rng(M * 1000003 + K * 131 + N)
    raw = blocks(fmt, rng, K, N, **PINS[fmt].get(pin, {}))
    a, b = parts(fmt, raw, K, N)
    x = rng.standard_normal((M, K)).astype(f32)
    got = qmatmul(be, QuantizedWeightUpload.from_gguf_blocks(raw, K, N, fmt), x, M, K, N, strided)
    pinned_values_hold(fmt, pin, raw, a, b, got)
    assert np.isfinite(got).all()
    check(got, x, a, b)


def form_program(fmt, K, N, block, nbytes):
    """one qmatmul over nbytes zero bytes handed over as file blocks of `block` elements"""
    qw = QuantizedWeightUpload(np.zeros(nbytes, np.uint8), np.zeros(0, f32), K, N, block, gguf=fmt)
    return DeviceProgram(ops=[DeviceOp.qmatmul(1, 0, 0, 1, N, K)], buffer_sizes=[K, N], qweights=[qw])


def model_config():
    """two layers, every projection width a multiple of 256, untied head: every projection and the head are super-blocks"""
    cfg = llama.preset("tiny")
    cfg.d_model, cfg.n_heads, cfg.n_kv_heads, cfg.d_ff, cfg.vocab_size, cfg.n_layers = 256, 4, 4, 512, 512, 2
    cfg.tied_lm_head = 0
    return cfg


# per gguf kind: the block bytes per weight (per layer q, k, v, o, gate, up, down; then the head) of model_config() (L/16 = L/8 = 0;
# layer 1 >= 7L/8 is a "more bits" layer of Q4_K_M / Q5_K_M, whose wv and w_down are Q6_K like the head)
MIXES = {llama.Q4_K_GGUF: [144] * 15,
         llama.Q4_K_M_GGUF: [144] * 7 + [144, 144, 210, 144, 144, 144, 210, 210],
         llama.Q5_K_M_GGUF: [176] * 7 + [176, 176, 210, 176, 176, 176, 210, 210],
         llama.Q3_K_M_GGUF: [110, 110, 176, 144, 110, 110, 144] * 2 + [210],
         llama.Q2_K_GGUF: [84, 84, 110, 110, 84, 84, 110] * 2 + [210]}
BY_BYTES = {row.nbytes: row for row in FORMATS.values()}
