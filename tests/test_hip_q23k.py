"""GGUF Q3_K / Q2_K weights on the MI355X (zgml_amd/csrc/sb_kernels.hip) against float64 over the dequantised weights (tests/q23k_cases.py). Per output
|y - ref| <= 2e-5 * sum_k |x[k]| * (|a| + |b|) + 1e-30, w = a - b: Q3_K (b = 0): Q6_K's bound over |w|; Q2_K: Q4_K's, over BOTH terms (summed apart)."""
import numpy as np
import pytest

from zgml_amd import DeviceOp, DeviceProgram, ProgramIO, QuantizedWeightUpload
from tests.q23k_cases import FORM_CASES, blocks, parts
from tests.q4k_cases import q4k_blocks, q4k_parts
from tests.test_hip_q4k import check, run

pytestmark = pytest.mark.gpu
f32 = np.float32
F16_MAX = 65504.0  # |w| <= 93 d: every f16 keeps the f32 sums of these shapes finite
# the largest finite weights (all bits set: Q3_K q = 3, sc - 32 = 31; Q2_K sc = m = 15, q = 3); every factor zero (Q3_K: every 6-bit
# scale 32); Q3_K q = 4 - 4 everywhere; Q3_K's low plane alone (q = low - 4); Q2_K's min term alone
PINS = {"q3_k": {"max": dict(d=-F16_MAX, hmask=0xFF, qs=0xFF, scales_lo=0xFF, scales_hi=0xFF), "zero": dict(scales_lo=0, scales_hi=0xAA),
                 "q zero": dict(qs=0, hmask=0xFF), "low only": dict(hmask=0)},
        "q2_k": {"max": dict(d=F16_MAX, dmin=-F16_MAX, scales=0xFF, qs=0xFF), "zero": dict(scales=0), "min only": dict(qs=0)}}
# tests/test_hip_q5k.py's shapes, for the reasons given there (the round is still the family's 256 k: no edge moves); then the pins
CASES = [(fmt, *c) for fmt in PINS for c in
         [(1, K, N, False, None) for K, N in [(1, 256), (37, 256), (257, 256), (4096, 512), (577, 768), (4097, 256)]] +
         [(M, K, N, False, None) for K, N in [(96, 256), (1001, 512)] for M in (2, 5, 16, 17, 33)] + [(5, 1000, 512, True, None)] +
         [(M, 96, 256, False, pin) for M in (1, 5) for pin in PINS[fmt]]]


@pytest.mark.parametrize("fmt,M,K,N,strided,pin", CASES)
def test_q23k_matmul_against_float64(hip_backend, fmt, M, K, N, strided, pin):
    rng = np.random.default_rng(M * 1000003 + K * 131 + N)
    raw = blocks(fmt, rng, K, N, **PINS[fmt].get(pin, {}))
    a, b = parts(fmt, raw, K, N)
    x = rng.standard_normal((M, K)).astype(f32)
    in_off, in_rs, dst_off, dst_rs = (3, K + 5, 7, N + 9) if strided else (0, K, 0, N)
    xin, ys = np.zeros(in_off + M * in_rs, f32), dst_off + M * dst_rs
    for m in range(M):
        xin[in_off + m * in_rs:][:K] = x[m]
    prog = DeviceProgram(ops=[DeviceOp.qmatmul(1, 0, 0, M, N, K, in_off, in_rs if strided else 0, dst_off, dst_rs if strided else 0)],
                         buffer_sizes=[xin.size, ys], initial_uploads=[ProgramIO(0, xin)],
                         qweights=[QuantizedWeightUpload.from_gguf_blocks(raw, K, N, fmt)])
    y = run(hip_backend, prog, [[(1, ys)]])[0][0]
    got = np.stack([y[dst_off + m * dst_rs:][:N] for m in range(M)])
    assert pin != "max" or (a.min() == a.max() == (-93 if fmt == "q3_k" else 45) * F16_MAX and b.min() == b.max() == (0 if fmt == "q3_k" else -15) * F16_MAX)
    assert pin not in ("zero", "q zero") or (not a.any() and not b.any() and not got.any())
    assert pin != "low only" or (a.any() and not raw[:, :32].any() and (np.sign(a[:, :16]) == np.sign(a[:, :1])).all())  # q = low - 4 < 0
    assert pin != "min only" or (not a.any() and got.any() and (b[:, :16] != b[:, 16:32]).any())
    assert np.isfinite(got).all()
    check(got, x, a, b)


def test_q23k_mixed_program_and_run_to_run_identity(hip_backend):  # each at a K-split shape, one execute; a second execute: same bytes
    rng = np.random.default_rng(11)
    shapes, kinds = [(577, 256), (577, 256), (261, 256)], ("q2_k", "q3_k", "q4_k")
    raws = [blocks("q2_k", rng, *shapes[0]), blocks("q3_k", rng, *shapes[1]), q4k_blocks(rng, *shapes[2])]
    xs = [rng.standard_normal(k).astype(f32) for k, _ in shapes]
    prog = DeviceProgram(ops=[DeviceOp.qmatmul(3 + i, i, i, 1, n, k) for i, (k, n) in enumerate(shapes)],
                         buffer_sizes=[k for k, _ in shapes] + [n for _, n in shapes], initial_uploads=[ProgramIO(i, x) for i, x in enumerate(xs)],
                         qweights=[QuantizedWeightUpload.from_gguf_blocks(r, *s, kind) for r, s, kind in zip(raws, shapes, kinds)])
    outs = [(3 + i, n) for i, (_, n) in enumerate(shapes)]
    first, second = run(hip_backend, prog, [outs, outs])
    refs = [parts("q2_k", raws[0], *shapes[0]), parts("q3_k", raws[1], *shapes[1]), q4k_parts(raws[2], *shapes[2])]
    for y, y2, x, (a, b) in zip(first, second, xs, refs):
        check(y[None, :], x[None, :], a, b)
        assert np.array_equal(y, y2)


@pytest.mark.parametrize("fmt", list(PINS))
def test_q23k_forms_the_device_takes(hip_backend, fmt):
    for K, N, block, nbytes, want in FORM_CASES[fmt]:
        p = DeviceProgram(ops=[DeviceOp.qmatmul(1, 0, 0, 1, N, K)], buffer_sizes=[K, N],
                          qweights=[QuantizedWeightUpload(np.zeros(nbytes, np.uint8), np.zeros(0, f32), K, N, block, gguf=fmt)])
        assert hip_backend._lib.zgml_hip_program_supported(p.to_c()[0]) == int(want), (K, N, block, nbytes)
