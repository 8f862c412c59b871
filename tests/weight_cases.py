"""Case table for the VALUE axis of the quantized mat-vec / matmul kernels: weight profiles (which scales and which stored
values a weight holds), weight format classes (what classify_kernel / gguf_form in zgml_amd/csrc make of an upload) and a float64
reference. No GPU and no HIP library here. Same role as attention_cases.py and handover_cases.py: tests/test_weight_cases_host.py
checks the table itself on any machine, tests/test_hip_weight_values.py runs it on the device.

Profiles, each (data int8 [K * N], scales f32 [ceil(K * N / bs)]) for a (K, N, rng, format class):
  positive     the generator every other test uses: scales rng.random().astype(f16) * c + 0.001 — the control
  negated      `positive` of the same seed with every scale negated
  gguf         a float matrix normal * exp(normal) * 0.02 * 2^U{-4..4} (per block), quantised per 32-element flat block by the
               published Q4_0 rule: d = v_max / -8 (v_max: the element of largest magnitude, so d is negative for half of the blocks)
               rounded to f16, q = clip(round(v / d) + 8, 0, 15) - 8, d == 0 -> stored nibble 8 everywhere. Q8 classes:
               d = amax / 127 with a random sign, q = clip(round(v / d), -127, 127). f32 classes keep d unrounded.
  extremes     scale magnitude constant per 32-column block-column j, cycling with (j + phase) % 6 through the f16 bit patterns
               0x0001 (smallest subnormal), 0x03FF (largest subnormal), 0x0400 (smallest normal), 0x3C00 (1.0), 0x6C00 (4096),
               0x0000 (zero), a random sign bit per block (so -0.0 occurs); f32 classes multiply by (1 + 2^-20), zeros excepted.
               Every output column sums ONE magnitude class, so the per-column bound cannot hide a small class behind a large
               one. A weight narrower than six block-columns cannot hold all six classes that way: `variants` gives the phases
               that together do (N = 32: six weights, N = 64: three), and a case runs every one of them. The raw class (blocks
               straddle columns) cycles by flat block index instead; its kernel is checked bit for bit against the oracle.
  zero_blocks  `positive` with a random third of the blocks at scale 0 or at all-zero data (stored nibble 8), and one whole
               block-column (N >= 64; the first 16-column group at N = 32; half the columns below) zeroed.
For the Q8 and raw classes every profile plants both -128 and 127 in the data (the ABI takes any int8).

Format classes: q4_f16, q4_f32 (values in [-8, 7], scales not f16-exact), q8_f16, q8_f32, raw (a shape that is not packable:
N % 32 != 0 or block size != 32), gguf_q4_0 / gguf_q8_0 (the f16 classes as raw file blocks through
QuantizedWeightUpload.from_gguf_blocks)."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

f32, f64 = np.float32, np.float64
TOL = 2e-5  # |got - want64| <= TOL * bound64 + FLOOR: the project's mat-vec contract
FLOOR = 1e-30
SENTINEL = -7.0

PROFILES = ("positive", "negated", "gguf", "extremes", "zero_blocks")
CLASSES = ("q4_f16", "q4_f32", "q8_f16", "q8_f32", "raw", "gguf_q4_0", "gguf_q8_0")
EXTREME_BITS = (0x0001, 0x03FF, 0x0400, 0x3C00, 0x6C00, 0x0000)


def is_q4(cls):
    return cls in ("q4_f16", "q4_f32", "gguf_q4_0")


def is_f16(cls):
    return cls in ("q4_f16", "q8_f16", "gguf_q4_0", "gguf_q8_0")


def f16_exact(scales):
    with np.errstate(over="ignore"):
        return scales.astype(np.float16).astype(f32) == scales


def _plant(data, rng, cls, keep_out=None):
    """Q8 / raw classes: both ends of int8 somewhere in the data (outside the columns `keep_out` = (N, c0, c1) keeps zero)"""
    if is_q4(cls):
        return
    idx = np.arange(data.size)
    if keep_out:
        N, c0, c1 = keep_out
        idx = idx[((idx % N) < c0) | ((idx % N) >= c1)]
    a, b = rng.choice(idx, 2, replace=False)
    data[a], data[b] = -128, 127


def _positive(K, N, rng, cls, bs):
    nb = (K * N + bs - 1) // bs
    c = 0.05 if is_q4(cls) else 0.01
    data = (rng.integers(-8, 8, K * N) if is_q4(cls) else rng.integers(-128, 128, K * N)).astype(np.int8)
    if is_f16(cls):
        scales = (rng.random(nb).astype(np.float16) * np.float16(c) + np.float16(0.001)).astype(f32)
    else:
        scales = (rng.random(nb) * c + 0.001).astype(f32)
    return data, scales


def _gguf(K, N, rng, cls, bs, amp=0.02):
    n = K * N
    nb = (n + bs - 1) // bs
    v = np.zeros(nb * bs, f64)
    v[:n] = rng.standard_normal(n) * np.exp(rng.standard_normal(n)) * amp
    v = v.reshape(nb, bs) * np.exp2(rng.integers(-4, 5, nb))[:, None]
    if is_q4(cls):
        v_max = v[np.arange(nb), np.argmax(np.abs(v), axis=1)]
        d = v_max / -8.0
    else:
        d = np.abs(v).max(axis=1) / 127.0 * rng.choice([-1.0, 1.0], nb)
    d = d.astype(np.float16).astype(f32) if is_f16(cls) else d.astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d[:, None] != 0, np.floor(v / d.astype(f64)[:, None] + 0.5), 0.0)
    q = np.clip(r + 8, 0, 15) - 8 if is_q4(cls) else np.clip(r, -127, 127)
    return q.astype(np.int8).ravel()[:n].copy(), d


def _extremes(K, N, rng, cls, bs, phase):
    nb = (K * N + bs - 1) // bs
    data = (rng.integers(-8, 8, K * N) if is_q4(cls) else rng.integers(-128, 128, K * N)).astype(np.int8)
    b = np.arange(nb)
    kind = (b % (N // 32) + phase) % 6 if (bs == 32 and N % 32 == 0) else (b + phase) % 6  # block b of a packable weight: j = b % NB
    bits = np.array(EXTREME_BITS, np.uint16)[kind] | (rng.integers(0, 2, nb).astype(np.uint16) << 15)
    scales = bits.view(np.float16).astype(f32)
    if not is_f16(cls):
        scales = (scales * f32(1.0 + 2.0 ** -20)).astype(f32)  # (zero stays zero)
    return data, scales


def zero_columns(N):
    """the output columns `zero_blocks` zeroes whole"""
    if N >= 64:
        j = (N // 32) // 2
        return 32 * j, 32 * j + 32
    return (0, 16) if N >= 32 else (0, max(1, N // 2))


def _zero_blocks(K, N, rng, cls, bs):
    data, scales = _positive(K, N, rng, cls, bs)
    nb = scales.size
    hit = rng.random(nb) < 1.0 / 3.0
    by_scale = rng.random(nb) < 0.5
    scales[hit & by_scale] = 0.0
    pad = np.zeros(nb * bs, np.int8)
    pad[:data.size] = data
    pad.reshape(nb, bs)[hit & ~by_scale] = 0
    data = pad[:K * N].copy()
    c0, c1 = zero_columns(N)
    if bs == 32 and N % 32 == 0 and c1 - c0 == 32:  # a whole block-column: through its scales in the upper half of K, its data below
        j = c0 // 32
        scales.reshape(K, N // 32)[: K // 2, j] = 0.0
        data.reshape(K, N)[K // 2:, c0:c1] = 0
    else:
        data.reshape(K, N)[:, c0:c1] = 0
    return data, scales


def variants(profile, N, bs=32):
    """the phases a case runs `profile` with: those of `extremes` that together show all six magnitude classes"""
    if profile != "extremes" or bs != 32 or N % 32 != 0:
        return [0]
    return list(range(0, 6, min(6, N // 32)))


def make(profile, cls, K, N, rng, bs=32, phase=0, packable=True, amp=0.02):
    """(data int8 [K * N], scales f32 [ceil(K * N / bs)]) of format class `cls` (amp: the amplitude of `gguf`'s float matrix)"""
    keep_out = None
    if profile == "positive":
        data, scales = _positive(K, N, rng, cls, bs)
    elif profile == "negated":
        data, scales = _positive(K, N, rng, cls, bs)
        scales = -scales
    elif profile == "gguf":
        data, scales = _gguf(K, N, rng, cls, bs, amp)
    elif profile == "extremes":
        data, scales = _extremes(K, N, rng, cls, bs, phase)
    elif profile == "zero_blocks":
        data, scales = _zero_blocks(K, N, rng, cls, bs)
        keep_out = (N, *zero_columns(N))
    else:
        raise ValueError(profile)
    _plant(data, rng, cls, keep_out)
    check_class(cls, data, scales, K, N, bs, packable)
    return data, scales


def check_class(cls, data, scales, K, N, bs, packable=True):
    """the upload really is of the class (what classify_kernel decides by: value range, f16 round trip of every scale)"""
    assert data.dtype == np.int8 and scales.dtype == f32 and data.size == K * N and scales.size == (K * N + bs - 1) // bs
    assert np.all(np.isfinite(scales))
    if cls == "raw":
        assert bs != 32 or N % 32 != 0
        return
    assert not packable or (bs == 32 and N % 32 == 0)
    if is_q4(cls):
        assert data.min() >= -8 and data.max() <= 7
    else:
        assert data.min() == -128 and data.max() == 127
    # (an f32-class weight of one block-column in the zero phase of `extremes` holds zeros only: the device files it under f16)
    assert bool(np.all(f16_exact(scales))) == is_f16(cls) or not np.any(scales)


def gguf_blocks(cls, data, scales):
    """raw file blocks of a gguf_* class weight"""
    from tests.synth import q4_0_blocks_from_int8, q8_0_blocks
    return q4_0_blocks_from_int8(data, scales) if cls == "gguf_q4_0" else q8_0_blocks(data, scales)


def reference(data, scales, x, M, N, K, bs=32):
    """dequantise and multiply in float64: (want64 [M, N], bound64 = |X| @ |W|)"""
    W = (data.astype(f64) * np.repeat(scales.astype(f64), bs)[:data.size]).reshape(K, N)
    X = np.asarray(x, f32).reshape(M, K).astype(f64)
    return X @ W, np.abs(X) @ np.abs(W)


# ── the route x class matrix of the device test ──────────────────────────────────────────────────────────────────────────
@dataclass(frozen=True)
class Case:
    route: str
    cls: str
    M: int
    K: int
    Ns: tuple            # one weight per entry; more than one: the grouped launch (same rows)
    bs: int = 32
    small_m: bool = False    # compile with OPT_SMALL_M_MATVEC = 8
    ordered: bool = False    # ordered fan-in: two executions agree bit for bit

    @property
    def id(self):
        return f"{self.route}-{self.cls}-M{self.M}-K{self.K}-N{'_'.join(map(str, self.Ns))}" + (f"-bs{self.bs}" if self.bs != 32 else "")

    @property
    def N(self):
        return self.Ns[0]

    @property
    def mfma(self):
        """the contraction runs on the matrix cores (every M > 1 form but the K-on-lanes rows and the raw kernel)"""
        return self.M > 1 and self.route not in ("kon-rows", "raw")


def _cases():
    out = []

    def add(route, classes, Ms, shapes, **kw):
        for cls in classes:
            for K, N in shapes:
                for M in Ms:
                    out.append(Case(route, cls, M, K, N if isinstance(N, tuple) else (N,), **kw))

    add("matvec-nol", ("q4_f16", "q4_f32", "q8_f16", "q8_f32"), (1,), [(32, 32), (100, 64), (576, 192)])
    add("matvec-kon", ("q4_f16", "gguf_q4_0"), (1,), [(2080, 32), (2051, 32), (4096, 64)])
    add("kon-rows", ("q4_f16",), (2, 8), [(2080, 32)], small_m=True)
    add("tile", ("q4_f32", "q8_f16", "q8_f32"), (2, 17), [(100, 64), (576, 192)])
    add("xdl2", ("q4_f16", "gguf_q4_0"), (2, 17, 32), [(100, 64), (576, 192)])
    add("xdl5", ("q4_f16",), (5, 32), [(576, 10240)], ordered=True)
    add("xdl4", ("q4_f16",), (33, 65), [(576, 64), (4096, 64)], ordered=True)
    add("xdl4-m32", ("q4_f16",), (32,), [(8192, 512)], ordered=True)
    add("grouped", ("q4_f16",), (1, 5), [(576, (576, 192, 192))])
    add("raw", ("raw",), (1, 3), [(64, 48)])
    add("raw", ("raw",), (1, 3), [(8, 8)], bs=4)
    add("gguf-pack", ("gguf_q4_0", "gguf_q8_0"), (1, 5), [(576, 192)])
    add("gguf-pack", ("gguf_q4_0", "gguf_q8_0"), (1,), [(2080, 32)])
    return out


CASES = _cases()
CASE_IDS = [c.id for c in CASES]
assert len(set(CASE_IDS)) == len(CASE_IDS)


@lru_cache(maxsize=12)
def weight(profile, cls, K, N, bs=32, part=0, phase=0):
    """the table's weight of that shape, deterministic (and shared between the cases that differ in M only; read-only):
    `negated` shares the seed of `positive`"""
    rng = np.random.default_rng([0x5CA1E, K, N, part, bs, CLASSES.index(cls)])
    data, scales = make(profile, cls, K, N, rng, bs, phase)
    data.setflags(write=False), scales.setflags(write=False)
    return data, scales


def case_weights(case, profile, phase=0):
    """[(data, scales)] per part of the case"""
    return [weight(profile, case.cls, case.K, N, case.bs, t, phase) for t, N in enumerate(case.Ns)]


def case_x(case):
    return np.random.default_rng([0xAC7, case.M, case.K]).standard_normal(case.M * case.K).astype(f32)


def distinct_weights():
    """(cls, K, N, bs, part) of every weight of the table, once"""
    return sorted({(c.cls, c.K, N, c.bs, t) for c in CASES for t, N in enumerate(c.Ns)})


# the W8A8 arm (tests/test_hip_w8a8.py): shapes x value kinds x profiles added to its bit-identity test
W8A8_SHAPES = ((64, 16), (576, 192))
W8A8_KINDS = ("q4_f16", "q8_f32")
W8A8_PROFILES = ("gguf", "negated")


def w8a8_weight(profile, kind, K, N):
    """(N = 16 is no packable width: only the value range and the scale format of the class are kept)"""
    rng = np.random.default_rng([0x8A8, K, N, CLASSES.index(kind)])
    return make(profile, kind, K, N, rng, 32, packable=N % 32 == 0)
