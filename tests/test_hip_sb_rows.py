"""The multi-row super-block mat-vecs (zgml_amd/csrc/sb_kernels.hip: sb_round_rows_kernel, sb4_rows_kernel; ZGML_HIP_OPT_SMALL_M_MATVEC):
2 <= M <= 8 rows over a Q4_K / Q5_K / Q6_K / Q3_K / Q2_K / IQ4_XS weight. Every row within the family's bound of float64
(sb_cases.check) and BIT-identical to the M = 1 launch over that row; the plan names the row launch exactly when it runs."""
import numpy as np
import pytest

from zgml_amd import DeviceOp, DeviceProgram, ProgramIO, QuantizedWeightUpload, capi
from tests import iq4xs_cases, sb_cases
from tests.sb_cases import F16_MAX, check, f32

pytestmark = pytest.mark.gpu
FORMATS = ["q4_k", "q5_k", "q6_k", "q3_k", "q2_k", "iq4_xs"]
TAG = {f: f.replace("_", "") + "-rows" for f in FORMATS}
# K below a sweep; a ragged K over three column blocks; one past sixteen rounds (two-round parts at the cap; Q4_K: its own split edge)
SHAPES = {f: [(37, 256), (577, 768), (261, 256) if f == "q4_k" else (4097, 256)] for f in FORMATS}
CASES = [(f, M, K, N, False) for f in FORMATS for M in (2, 3, 4, 5, 8) for K, N in SHAPES[f]] + [(f, 5, 1000, 512, True) for f in FORMATS]


def weight(fmt, rng, K, N, pin=None):
    """(upload, a, b) of seeded blocks: w = a - b in float64"""
    if fmt == "iq4_xs":
        raw = iq4xs_cases.iq4xs_blocks(rng, K, N, **iq4xs_cases.PINS.get(pin, {}))
        a, b = iq4xs_cases.iq4xs_parts(raw, K, N)
    else:
        raw = sb_cases.blocks(fmt, rng, K, N, **sb_cases.PINS[fmt].get(pin, {}))
        a, b = sb_cases.parts(fmt, raw, K, N)
    return QuantizedWeightUpload.from_gguf_blocks(raw, K, N, fmt), raw, a, b


def program(qw, x, M, K, N, strided=False, rows=None):
    """one qmatmul of M rows (buffers sized for `rows`), sb_cases.qmatmul's offsets and strides -> (program, op of m rows, rows of a read-back)"""
    rows = rows or M
    in_off, in_rs, dst_off, dst_rs = (3, K + 5, 7, N + 9) if strided else (0, K, 0, N)
    xin, ys = np.zeros(in_off + rows * in_rs, f32), dst_off + rows * dst_rs
    for m in range(len(x)):
        xin[in_off + m * in_rs:][:K] = x[m]
    op = lambda m: DeviceOp.qmatmul(1, 0, 0, m, N, K, in_off, in_rs if strided else 0, dst_off, dst_rs if strided else 0)
    cut = lambda y, m: np.stack([y[dst_off + r * dst_rs:][:N] for r in range(m)])
    return DeviceProgram(ops=[op(M)], buffer_sizes=[xin.size, ys], initial_uploads=[ProgramIO(0, xin)], qweights=[qw]), op, cut, ys


def compiled(be, prog, value):
    be.set_option(capi.OPT_SMALL_M_MATVEC, value)
    try:
        h = be.compileProgram(prog)
    finally:
        be.set_option(capi.OPT_SMALL_M_MATVEC, 0)
    assert h, be.last_error()
    return h


def execute(be, h, ys):
    y = np.zeros(ys, f32)
    be.executeProgram(h, [], [ProgramIO(1, y)])
    assert not be.last_error(), be.last_error()
    return y


@pytest.mark.parametrize("fmt,M,K,N,strided", CASES)
def test_rows_against_float64_and_the_single_row_launch(hip_backend, fmt, M, K, N, strided):
    rng = np.random.default_rng(M * 1000003 + K * 131 + N)
    qw, _, a, b = weight(fmt, rng, K, N)
    x = rng.standard_normal((M, K)).astype(f32)
    prog, _, cut, ys = program(qw, x, M, K, N, strided)
    h = compiled(hip_backend, prog, 8)
    try:
        assert TAG[fmt] in hip_backend.planText(h)  # (a)
        first, second = execute(hip_backend, h, ys), execute(hip_backend, h, ys)
    finally:
        hip_backend.freeProgram(h)
    got = cut(first, M)
    check(got, x, a, b)  # (b)
    for m in range(M):  # (c): the option at 0 (the default)
        assert np.array_equal(got[m], sb_cases.qmatmul(hip_backend, qw, x[m:m + 1], 1, K, N)[0]), m
    assert np.array_equal(first, second)  # (d)


@pytest.mark.parametrize("fmt,pin", [(f, pin) for f in FORMATS for pin in ("max", "mirror" if f == "q4_k" else "zero")])  # (Q4_K's zero pin: a = 0)
def test_pins(hip_backend, fmt, pin):
    M, K, N = 3, 96, 256
    rng = np.random.default_rng(M * 1000003 + K * 131 + N)
    qw, raw, a, b = weight(fmt, rng, K, N, pin)
    x = rng.standard_normal((M, K)).astype(f32)
    prog, _, cut, ys = program(qw, x, M, K, N)
    h = compiled(hip_backend, prog, 8)
    try:
        assert TAG[fmt] in hip_backend.planText(h)
        got = cut(execute(hip_backend, h, ys), M)
    finally:
        hip_backend.freeProgram(h)
    if fmt != "iq4_xs":
        sb_cases.pinned_values_hold(fmt, pin, raw, a, b, got)
    elif pin == "max":
        assert a.min() == a.max() == 4064 * F16_MAX
    else:
        assert not a.any() and not got.any()
    assert np.isfinite(got).all()
    check(got, x, a, b)


@pytest.mark.parametrize("fmt", FORMATS)
def test_option_one_routes_two_rows(hip_backend, fmt):
    """the option's value 1 (what BatchSession sets): every format's measured bound is >= 2, so M = 2 takes the row launch"""
    M, K, N = 2, 96, 256
    rng = np.random.default_rng(K * 131 + N)
    qw, _, a, b = weight(fmt, rng, K, N)
    x = rng.standard_normal((M, K)).astype(f32)
    prog, _, cut, ys = program(qw, x, M, K, N)
    h = compiled(hip_backend, prog, 1)
    try:
        assert TAG[fmt] in hip_backend.planText(h)
        check(cut(execute(hip_backend, h, ys), M), x, a, b)
    finally:
        hip_backend.freeProgram(h)


def test_refresh_below_and_above_the_bound(hip_backend):
    """compiled at M = 4 under the option at 4: M = 2 keeps the row launch (its scratch is there), M = 9 runs the matmul kernel"""
    fmt, K, N = "q5_k", 577, 768
    rng = np.random.default_rng(9)
    qw, _, a, b = weight(fmt, rng, K, N)
    x = rng.standard_normal((9, K)).astype(f32)
    prog, op, cut, ys = program(qw, x, 4, K, N, rows=9)
    h = compiled(hip_backend, prog, 4)
    try:
        for M, tag in ((4, TAG[fmt]), (2, TAG[fmt]), (9, "q5k-matmul")):
            hip_backend.refreshProgram(h, [op(M)])
            assert not hip_backend.last_error(), hip_backend.last_error()
            got = cut(execute(hip_backend, h, ys), M)
            assert tag in hip_backend.planText(h), (M, hip_backend.planText(h))
            check(got, x[:M], a, b)
    finally:
        hip_backend.freeProgram(h)
