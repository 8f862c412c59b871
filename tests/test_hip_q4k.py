"""GGUF Q4_K weights on the MI355X (zgml_amd/csrc/sb_kernels.hip) against float64 over the dequantised weights (tests/q4k_cases.py).
Per output |y - ref| <= 2e-5 * sum_k |x[k]| * (|d sc q| + |dmin m|) + 1e-30: the project's mat-vec bound, its magnitude over BOTH
terms (the kernels sum them apart, and they cancel in w)."""
import numpy as np
import pytest

from zgml_amd import DeviceOp, DeviceProgram, ProgramIO, QuantizedWeightUpload
from tests.q4k_cases import q4k_blocks, q4k_parts
from tests.synth import q4_0_blocks_from_int8

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
F16_MAX = 65504.0  # w <= 1008 d: every f16 keeps the f32 sums of these shapes finite


def run(be, prog, outs):
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
    x = x.astype(f64)
    assert np.all(np.abs(got - x @ (a - b)) <= 2e-5 * (np.abs(x) @ (np.abs(a) + np.abs(b))) + 1e-30)


def qmatmul_q4k(be, raw, x, M, K, N, in_off=0, in_rs=0, dst_off=0, dst_rs=0):
    xs, ys = in_off + (M - 1) * (in_rs or K) + K, dst_off + (M - 1) * (dst_rs or N) + N
    xin = np.zeros(xs, f32)
    for m in range(M):
        xin[in_off + m * (in_rs or K):][:K] = x[m]
    prog = DeviceProgram(ops=[DeviceOp.qmatmul(1, 0, 0, M, N, K, in_off, in_rs, dst_off, dst_rs)], buffer_sizes=[xs, ys],
                         initial_uploads=[ProgramIO(0, xin)], qweights=[QuantizedWeightUpload.from_gguf_blocks(raw, K, N, "q4_k")])
    y = run(be, prog, [[(1, ys)]])[0][0]
    return np.stack([y[dst_off + m * (dst_rs or N):][:N] for m in range(M)])


# M = 1: one super-block column and one k; K odd, below one sweep; K one past the 256-k share of a part (the split and its combine
# with a ragged last part); a Llama-like shape (16 parts); three super-block columns with K no multiple of 64. M > 1: rows below, at
# and over the 16-row tile at a K of one and a half chunks and a K that is no multiple of 8; one case with strides and offsets.
# Extremes (q_byte set): every q = 15, and its mirror q = 0, with sc = m = 63, d the largest f16 and dmin = -d.
CASES = [(1, K, N, False, None) for K, N in [(1, 256), (37, 256), (261, 256), (4096, 512), (577, 768)]] + \
        [(M, K, N, False, None) for K, N in [(96, 256), (1000, 512)] for M in (2, 5, 16, 17, 33)] + [(5, 1000, 512, True, None)] + \
        [(M, 96, 256, False, qb) for M in (1, 5) for qb in (0xFF, 0x00)]


@pytest.mark.parametrize("M,K,N,strided,q_byte", CASES)
def test_q4k_matmul_against_float64(hip_backend, M, K, N, strided, q_byte):
    rng = np.random.default_rng(M * 1000003 + K * 131 + N)
    pin = {} if q_byte is None else dict(d=F16_MAX, dmin=-F16_MAX, scale_byte=0xFF, q_byte=q_byte)
    raw = q4k_blocks(rng, K, N, **pin)
    a, b = q4k_parts(raw, K, N)
    if pin:
        assert a.max() == (63 * 15 * F16_MAX if q_byte else 0) and b.min() == b.max() == -63 * F16_MAX
    x = rng.standard_normal((M, K)).astype(f32)
    kw = dict(in_off=3, in_rs=K + 5, dst_off=7, dst_rs=N + 9) if strided else {}
    got = qmatmul_q4k(hip_backend, raw, x, M, K, N, **kw)
    assert np.isfinite(got).all()
    check(got, x, a, b)


def test_q4k_mixed_program_and_run_to_run_identity(hip_backend):
    """Q4_K (at the K-split shape), Q4_0 pass-through and raw weights in one program and one execute; a second execute: same bytes"""
    rng = np.random.default_rng(11)
    shapes = [(261, 256), (64, 96), (64, 24)]
    raw_k = q4k_blocks(rng, *shapes[0])
    d0 = rng.integers(-8, 8, 64 * 96).astype(np.int8)
    s0 = (rng.random(64 * 96 // 32).astype(np.float16) * 0.05 + 0.001).astype(f32)
    d1 = rng.integers(-127, 128, 64 * 24).astype(np.int8)  # N = 24: not packable, stays raw
    s1 = (rng.random(64 * 24 // 32) * 0.01 + 0.001).astype(f32)
    xs = [rng.standard_normal(k).astype(f32) for k, _ in shapes]
    qws = [QuantizedWeightUpload.from_gguf_blocks(raw_k, *shapes[0], "q4_k"),
           QuantizedWeightUpload.from_gguf_blocks(q4_0_blocks_from_int8(d0, s0), 64, 96, "q4_0"), QuantizedWeightUpload(d1, s1, 64, 24, 32)]
    prog = DeviceProgram(ops=[DeviceOp.qmatmul(3 + i, i, i, 1, n, k) for i, (k, n) in enumerate(shapes)],
                         buffer_sizes=[k for k, _ in shapes] + [n for _, n in shapes],
                         initial_uploads=[ProgramIO(i, x) for i, x in enumerate(xs)], qweights=qws)
    outs = [(3 + i, n) for i, (_, n) in enumerate(shapes)]
    first, second = run(hip_backend, prog, [outs, outs])
    zero = np.zeros((64, 1))
    parts = [q4k_parts(raw_k, *shapes[0]), ((d0.astype(f64) * np.repeat(s0.astype(f64), 32)).reshape(64, 96), zero),
             ((d1.astype(f64) * np.repeat(s1.astype(f64), 32)).reshape(64, 24), zero)]
    for y, y2, x, (a, b) in zip(first, second, xs, parts):
        check(y[None, :], x[None, :], a, b)
        assert np.array_equal(y, y2)


def test_q4k_form_is_told_by_block_size(hip_backend):
    """the same bytes with block_size 32 give Q4_0's numbers; block_size 256 with cols % 256 != 0 or a byte too many is no form"""
    rng = np.random.default_rng(5)
    K, N = 64, 256
    d0 = rng.integers(-8, 8, K * N).astype(np.int8)
    s0 = (rng.random(K * N // 32).astype(np.float16) * 0.05 + 0.001).astype(f32)
    raw = q4_0_blocks_from_int8(d0, s0)
    assert raw.size == K * N // 256 * 144
    x = rng.standard_normal(K).astype(f32)
    prog = DeviceProgram(ops=[DeviceOp.qmatmul(1, 0, 0, 1, N, K)], buffer_sizes=[K, N], initial_uploads=[ProgramIO(0, x)],
                         qweights=[QuantizedWeightUpload.from_gguf_blocks(raw, K, N, "q4_0")])
    y = run(hip_backend, prog, [[(1, N)]])[0][0]
    check(y[None, :], x[None, :], (d0.astype(f64) * np.repeat(s0.astype(f64), 32)).reshape(K, N), np.zeros((K, 1)))
    supported = hip_backend._lib.zgml_hip_program_supported
    for k, n, extra in [(64, 256, 0), (64, 384, 0), (64, 256, 1)]:
        qw = QuantizedWeightUpload(np.zeros(k * n // 256 * 144 + extra, np.uint8), np.zeros(0, f32), k, n, 256, gguf="q4_k")
        p = DeviceProgram(ops=[DeviceOp.qmatmul(1, 0, 0, 1, n, k)], buffer_sizes=[k, n], qweights=[qw])
        assert supported(p.to_c()[0]) == (1 if (n, extra) == (256, 0) else 0), (k, n, extra)
