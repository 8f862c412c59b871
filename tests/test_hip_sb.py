"""GGUF super-block weights (Q2_K .. Q6_K) on the MI355X (zgml_amd/csrc/sb_kernels.hip): programs that mix them and the upload forms the
device takes. Per output |y - ref| <= 2e-5 * sum_k |x[k]| * (|a| + |b|) + 1e-30 with w = a - b: sb_cases.check. The matmul cases
of each format: tests/test_hip_q4k.py, _q5k.py, _q6k.py, _q23k.py over sb_cases.matmul_against_float64."""
import numpy as np
import pytest

from zgml_amd import DeviceOp, DeviceProgram, ProgramIO, QuantizedWeightUpload
from tests.sb_cases import FORM_CASES, FORMATS, blocks, check, form_program, parts, run
from tests.synth import q4_0_blocks_from_int8

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


def mixed_weight(kind, rng, K, N):
    """the upload and the float64 pair (a, b) of one weight of a mixed program: a super-block format, Q4_0 file blocks or the raw form"""
    if kind in FORMATS:
        raw = blocks(kind, rng, K, N)
        return QuantizedWeightUpload.from_gguf_blocks(raw, K, N, kind), parts(kind, raw, K, N)
    if kind == "q4_0":
        d = rng.integers(-8, 8, K * N).astype(np.int8)
        s = (rng.random(K * N // 32).astype(np.float16) * 0.05 + 0.001).astype(f32)
        qw = QuantizedWeightUpload.from_gguf_blocks(q4_0_blocks_from_int8(d, s), K, N, "q4_0")
    else:
        d = rng.integers(-127, 128, K * N).astype(np.int8)
        s = (rng.random(K * N // 32) * 0.01 + 0.001).astype(f32)
        qw = QuantizedWeightUpload(d, s, K, N, 32)
    return qw, ((d.astype(f64) * np.repeat(s.astype(f64), 32)).reshape(K, N), np.zeros((K, 1)))


# the super-block weights at a K-split shape each (Q4_K's own: 261); N = 24 is not packable and stays raw
@pytest.mark.parametrize("weights", [[("q4_k", 261, 256), ("q4_0", 64, 96), ("raw", 64, 24)], [("q6_k", 577, 256), ("q4_k", 261, 256), ("raw", 64, 24)],
                                     [("q5_k", 577, 256), ("q6_k", 577, 256), ("q4_k", 261, 256)], [("q2_k", 577, 256), ("q3_k", 577, 256), ("q4_k", 261, 256)]],
                         ids=lambda w: "+".join(kind for kind, _, _ in w))
def test_mixed_program_and_run_to_run_identity(hip_backend, weights):
    """several kinds of weight in one program and one execute (what shares scratch with what); a second execute: the same bytes"""
    rng = np.random.default_rng(11)
    qws, refs = zip(*[mixed_weight(kind, rng, K, N) for kind, K, N in weights])
    xs = [rng.standard_normal(K).astype(f32) for _, K, _ in weights]
    n = len(weights)
    prog = DeviceProgram(ops=[DeviceOp.qmatmul(n + i, i, i, 1, N, K) for i, (_, K, N) in enumerate(weights)],
                         buffer_sizes=[K for _, K, _ in weights] + [N for _, _, N in weights],
                         initial_uploads=[ProgramIO(i, x) for i, x in enumerate(xs)], qweights=list(qws))
    outs = [(n + i, N) for i, (_, _, N) in enumerate(weights)]
    first, second = run(hip_backend, prog, [outs, outs])
    for y, y2, x, (a, b) in zip(first, second, xs, refs):
        check(y[None, :], x[None, :], a, b)
        assert np.array_equal(y, y2)


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_forms_the_device_takes(hip_backend, fmt):
    for K, N, block, nbytes, want in FORM_CASES[fmt]:
        p = form_program(fmt, K, N, block, nbytes)
        assert hip_backend._lib.zgml_hip_program_supported(p.to_c()[0]) == int(want), (K, N, block, nbytes)


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
