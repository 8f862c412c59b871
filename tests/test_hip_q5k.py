"""GGUF Q5_K weights on the MI355X (zgml_amd/csrc/sb_kernels.hip) against float64 over the dequantised weights (tests/q5k_cases.py). Per output
|y - ref| <= 2e-5 * sum_k |x[k]| * (|d sc q| + |dmin m|) + 1e-30: Q4_K's bound, over BOTH terms (summed apart, they cancel in w)."""
import numpy as np
import pytest

from zgml_amd import DeviceOp, DeviceProgram, ProgramIO, QuantizedWeightUpload
from tests.q4k_cases import q4k_blocks, q4k_parts
from tests.q5k_cases import FORM_CASES, q5k_blocks, q5k_parts
from tests.q6k_cases import q6k_blocks, q6k_weights
from tests.test_hip_q4k import check, run

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
F16_MAX = 65504.0  # w <= 63 * 32 d: every f16 keeps the f32 sums of these shapes finite

PINS = {None: {}, "max": dict(d=F16_MAX, dmin=-F16_MAX, scale_byte=0xFF, ql_byte=0xFF, qh_byte=0xFF),
        "high only": dict(ql_byte=0, qh_byte=0xFF), "zero": dict(scale_byte=0)}
# M = 1 (kSbRound = 256 k, kSbSweep = 64, kSbRoundMaxParts = 16): one column block and one k; K odd, below a sweep; K one past a one-round
# share (two parts, the last of one k); 16 rounds over two column blocks (16 parts of one round: the cap); three column blocks, K no
# multiple of the sweep; K one past 16 rounds (the cap makes parts of two rounds). M > 1 (row tile 16, two per workgroup over M = 16;
# chunk 64 k dealt to 8 waves): K of 1.5 chunks; K no multiple of 8 over two column blocks (16 chunks: two per wave); strides and
# offsets. Pins: the largest finite weights; q = 16 everywhere (the high plane alone); sc = m = 0.
CASES = [(1, K, N, False, None) for K, N in [(1, 256), (37, 256), (257, 256), (4096, 512), (577, 768), (4097, 256)]] + \
        [(M, K, N, False, None) for K, N in [(96, 256), (1001, 512)] for M in (2, 5, 16, 17, 33)] + [(5, 1000, 512, True, None)] + \
        [(M, 96, 256, False, pin) for M in (1, 5) for pin in ("max", "high only", "zero")]


@pytest.mark.parametrize("M,K,N,strided,pin", CASES)
def test_q5k_matmul_against_float64(hip_backend, M, K, N, strided, pin):
    rng = np.random.default_rng(M * 1000003 + K * 131 + N)
    raw = q5k_blocks(rng, K, N, **PINS[pin])
    a, b = q5k_parts(raw, K, N)
    x = rng.standard_normal((M, K)).astype(f32)
    in_off, in_rs, dst_off, dst_rs = (3, K + 5, 7, N + 9) if strided else (0, K, 0, N)
    xin, ys = np.zeros(in_off + M * in_rs, f32), dst_off + M * dst_rs
    for m in range(M):
        xin[in_off + m * in_rs:][:K] = x[m]
    prog = DeviceProgram(ops=[DeviceOp.qmatmul(1, 0, 0, M, N, K, in_off, in_rs if strided else 0, dst_off, dst_rs if strided else 0)],
                         buffer_sizes=[xin.size, ys], initial_uploads=[ProgramIO(0, xin)],
                         qweights=[QuantizedWeightUpload.from_gguf_blocks(raw, K, N, "q5_k")])
    y = run(hip_backend, prog, [[(1, ys)]])[0][0]
    got = np.stack([y[dst_off + m * dst_rs:][:N] for m in range(M)])
    assert pin != "max" or (a.min() == a.max() == 63 * 31 * F16_MAX and b.min() == b.max() == -63 * F16_MAX)
    ones = np.concatenate([raw[:, :16], np.full((len(raw), 128), 0x11, np.uint8)], axis=1)  # the same headers over Q4_K nibbles of 1: d * sc
    assert pin != "high only" or (a.any() and np.array_equal(a, 16 * q4k_parts(ones, K, N)[0]))
    assert pin != "zero" or (not a.any() and not b.any() and not got.any())
    assert np.isfinite(got).all()
    check(got, x, a, b)


def test_q5k_mixed_program_and_run_to_run_identity(hip_backend):
    """Q5_K, Q6_K and Q4_K, each at a K-split shape, in one program and one execute; a second execute: same bytes"""
    rng = np.random.default_rng(11)
    shapes = [(577, 256), (577, 256), (261, 256)]
    raws = [q5k_blocks(rng, *shapes[0]), q6k_blocks(rng, *shapes[1]), q4k_blocks(rng, *shapes[2])]
    xs = [rng.standard_normal(k).astype(f32) for k, _ in shapes]
    qws = [QuantizedWeightUpload.from_gguf_blocks(r, *s, kind) for r, s, kind in zip(raws, shapes, ("q5_k", "q6_k", "q4_k"))]
    prog = DeviceProgram(ops=[DeviceOp.qmatmul(3 + i, i, i, 1, n, k) for i, (k, n) in enumerate(shapes)],
                         buffer_sizes=[k for k, _ in shapes] + [n for _, n in shapes],
                         initial_uploads=[ProgramIO(i, x) for i, x in enumerate(xs)], qweights=qws)
    outs = [(3 + i, n) for i, (_, n) in enumerate(shapes)]
    first, second = run(hip_backend, prog, [outs, outs])
    parts = [q5k_parts(raws[0], *shapes[0]), (q6k_weights(raws[1], *shapes[1]), np.zeros((577, 1))), q4k_parts(raws[2], *shapes[2])]
    for y, y2, x, (a, b) in zip(first, second, xs, parts):
        check(y[None, :], x[None, :], a, b)
        assert np.array_equal(y, y2)


def test_q5k_forms_the_device_takes(hip_backend):
    for K, N, block, nbytes, want in FORM_CASES:
        qw = QuantizedWeightUpload(np.zeros(nbytes, np.uint8), np.zeros(0, f32), K, N, block, gguf="q5_k")
        p = DeviceProgram(ops=[DeviceOp.qmatmul(1, 0, 0, 1, N, K)], buffer_sizes=[K, N], qweights=[qw])
        assert hip_backend._lib.zgml_hip_program_supported(p.to_c()[0]) == int(want), (K, N, block, nbytes)
