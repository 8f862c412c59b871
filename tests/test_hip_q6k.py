"""GGUF Q6_K weights on the MI355X (zgml_amd/csrc/sb_kernels.hip) against float64 over the dequantised weights (tests/q6k_cases.py).
Per output |y - ref| <= 2e-5 * sum_k |x[k]| |w[k, n]| + 1e-30: the project's mat-vec bound as it is, which is zero where w is."""
import numpy as np
import pytest

from zgml_amd import DeviceOp, DeviceProgram, ProgramIO, QuantizedWeightUpload
from tests.q4k_cases import q4k_blocks, q4k_parts
from tests.q6k_cases import FORM_CASES, q6k_blocks, q6k_weights
from tests.test_hip_q4k import run

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
F16_MAX = 65504.0


def check(got, x, w, mag=None):
    x = x.astype(f64)
    assert np.all(np.abs(got - x @ w) <= 2e-5 * (np.abs(x) @ (np.abs(w) if mag is None else mag)) + 1e-30)


# M = 1 (round 256 k, sweep 64): one column block and one k; K odd, below a sweep; K one past a one-round share (split, ragged last
# part); 16 parts; three column blocks, K no multiple of 64; K one past sixteen rounds (parts of two rounds). M > 1 (row tile 16, two
# per workgroup over M = 16; chunk 64): K of 1.5 chunks and K no multiple of 8; strides and offsets. Extremes: q = 0 at the largest d, q = 32.
CASES = [(1, K, N, False, None) for K, N in [(1, 256), (37, 256), (257, 256), (4096, 512), (577, 768), (4097, 256)]] + \
        [(M, K, N, False, None) for K, N in [(96, 256), (1001, 512)] for M in (2, 5, 16, 17, 33)] + [(5, 1000, 512, True, None)] + \
        [(M, 96, 256, False, pin) for M in (1, 5) for pin in ("max", "zero")]


@pytest.mark.parametrize("M,K,N,strided,pin", CASES)
def test_q6k_matmul_against_float64(hip_backend, M, K, N, strided, pin):
    rng = np.random.default_rng(M * 1000003 + K * 131 + N)
    kw = {"max": dict(d=F16_MAX, scale=-128, ql_byte=0, qh_byte=0), "zero": dict(ql_byte=0, qh_byte=0xAA), None: {}}[pin]
    raw = q6k_blocks(rng, K, N, **kw)
    w = q6k_weights(raw, K, N)
    x = rng.standard_normal((M, K)).astype(f32)
    in_off, in_rs, dst_off, dst_rs = (3, K + 5, 7, N + 9) if strided else (0, K, 0, N)
    xin, ys = np.zeros(in_off + M * in_rs, f32), dst_off + M * dst_rs
    for m in range(M):
        xin[in_off + m * in_rs:][:K] = x[m]
    prog = DeviceProgram(ops=[DeviceOp.qmatmul(1, 0, 0, M, N, K, in_off, in_rs if strided else 0, dst_off, dst_rs if strided else 0)],
                         buffer_sizes=[xin.size, ys], initial_uploads=[ProgramIO(0, xin)],
                         qweights=[QuantizedWeightUpload.from_gguf_blocks(raw, K, N, "q6_k")])
    y = run(hip_backend, prog, [[(1, ys)]])[0][0]
    got = np.stack([y[dst_off + m * dst_rs:][:N] for m in range(M)])
    assert pin != "max" or (w.min() == w.max() == F16_MAX * 128 * 32 and np.isfinite(got).all())
    assert pin != "zero" or (not w.any() and not got.any())
    check(got, x, w)


def test_q6k_mixed_program_and_run_to_run_identity(hip_backend):
    """Q6_K and Q4_K (both at a K-split shape) and a raw weight in one program and one execute; a second execute: same bytes"""
    rng = np.random.default_rng(11)
    shapes = [(577, 256), (261, 256), (64, 24)]
    raw6, raw4 = q6k_blocks(rng, *shapes[0]), q4k_blocks(rng, *shapes[1])
    d1 = rng.integers(-127, 128, 64 * 24).astype(np.int8)  # N = 24: not packable, stays raw
    s1 = (rng.random(64 * 24 // 32) * 0.01 + 0.001).astype(f32)
    xs = [rng.standard_normal(k).astype(f32) for k, _ in shapes]
    qws = [QuantizedWeightUpload.from_gguf_blocks(raw6, *shapes[0], "q6_k"), QuantizedWeightUpload.from_gguf_blocks(raw4, *shapes[1], "q4_k"),
           QuantizedWeightUpload(d1, s1, 64, 24, 32)]
    prog = DeviceProgram(ops=[DeviceOp.qmatmul(3 + i, i, i, 1, n, k) for i, (k, n) in enumerate(shapes)],
                         buffer_sizes=[k for k, _ in shapes] + [n for _, n in shapes],
                         initial_uploads=[ProgramIO(i, x) for i, x in enumerate(xs)], qweights=qws)
    outs = [(3 + i, n) for i, (_, n) in enumerate(shapes)]
    first, second = run(hip_backend, prog, [outs, outs])
    a, b = q4k_parts(raw4, *shapes[1])
    w1 = (d1.astype(f64) * np.repeat(s1.astype(f64), 32)).reshape(64, 24)
    for y, y2, x, (w, mag) in zip(first, second, xs, [(q6k_weights(raw6, *shapes[0]), None), (a - b, np.abs(a) + np.abs(b)), (w1, None)]):
        check(y[None, :], x[None, :], w, mag)
        assert np.array_equal(y, y2)


@pytest.mark.parametrize("K,N,block,nbytes,want", FORM_CASES)
def test_q6k_forms_the_device_takes(hip_backend, K, N, block, nbytes, want):
    qw = QuantizedWeightUpload(np.zeros(nbytes, np.uint8), np.zeros(0, f32), K, N, block, gguf="q6_k")
    p = DeviceProgram(ops=[DeviceOp.qmatmul(1, 0, 0, 1, N, K)], buffer_sizes=[K, N], qweights=[qw])
    assert hip_backend._lib.zgml_hip_program_supported(p.to_c()[0]) == int(want)
