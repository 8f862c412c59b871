"""The multi-row K-on-lanes Q4_0 mat-vec (zgml_amd/csrc/qmatvec_rows.hip, ZGML_HIP_OPT_SMALL_M_MATVEC): 2 <= M <= 8 rows over a
long-K GGUF-valued Q4_0 weight with f16 scales, every row within the project's mat-vec contract
|delta| <= 2e-5 * sum_k |x_k * w_kn| of the oracle's exact path — and the routing around it: off by default (tile kernels, same
contract), on: K-on-lanes layout for weights every use of which has M <= the bound, a later larger M refused at refresh_program.
The option's value 1 routes M <= 6 (the measured bound); the kernel itself goes to 8 rows (value 8)."""
import numpy as np
import pytest

from zgml_amd import DeviceOp, DeviceProgram, ProgramIO, QuantizedWeightUpload, capi
from tests.test_hip_qmatvec import TOL, bound, run_both

pytestmark = pytest.mark.gpu
f32 = np.float32
ROWS_TAG = "qmatvec-kon-rows"


@pytest.fixture
def small_m(hip_backend):
    hip_backend.set_option(capi.OPT_SMALL_M_MATVEC, 8)  # the kernel at every row count it is built for
    yield hip_backend
    hip_backend.set_option(capi.OPT_SMALL_M_MATVEC, 0)


def q4_case(seed, M, K, N):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(M * K).astype(f32)
    data = rng.integers(-8, 8, K * N).astype(np.int8)
    scales = (rng.random((K * N + 31) // 32).astype(np.float16) * 0.05 + 0.001).astype(f32)  # f16-exact: what a GGUF block holds
    return x, data, scales


def program(data, scales, x, M, N, K, in_off=0, in_rs=0, dst_off=0, dst_rs=0):
    xin = np.full(in_off + (M - 1) * (in_rs or K) + K + 3, 99, f32)
    for m in range(M):
        xin[in_off + m * (in_rs or K):][:K] = x.reshape(M, K)[m]
    dst_len = dst_off + (M - 1) * (dst_rs or N) + N + 2
    return DeviceProgram(ops=[DeviceOp.qmatmul(1, 0, 0, M, N, K, in_off, in_rs, dst_off, dst_rs)], buffer_sizes=[xin.size, dst_len],
                         initial_uploads=[ProgramIO(0, xin), ProgramIO(1, np.full(dst_len, -7, f32))],
                         qweights=[QuantizedWeightUpload(data, scales, K, N, 32)]), dst_len


def plan_of(be, prog):
    h = be.compileProgram(prog)
    assert h, be.last_error()
    try:
        return be.planText(h)
    finally:
        be.freeProgram(h)


def check_rows(got, want, data, scales, x, M, N, K, dst_off=0, dst_rs=0):
    bb = bound(data, scales, x, M, N, K, 32)
    worst = 0.0
    for m in range(M):
        lo = dst_off + m * (dst_rs or N)
        d = np.abs(got[lo:lo + N].astype(np.float64) - want[lo:lo + N])
        worst = max(worst, float(np.max(d / (bb[m] + 1e-30))))
        assert np.all(d <= TOL * bb[m] + 1e-30), (m, worst)
    assert np.array_equal(got == -7, want == -7)  # sentinels in front of, between and behind the rows untouched
    return worst


@pytest.mark.parametrize("M", [2, 3, 4, 5, 7, 8])
@pytest.mark.parametrize("K,N", [(4096, 4096), (4096, 11008), (11008, 4096)])
def test_rows_kernel_matches_oracle(small_m, oracle, K, N, M):
    oracle.set_threads(16)
    x, data, scales = q4_case(0x20A5 + M + K + 3 * N, M, K, N)
    prog, _ = program(data, scales, x, M, N, K)
    assert ROWS_TAG in plan_of(small_m, prog)
    want, got = run_both(small_m, oracle, data, scales, x, M, N, K)
    assert not small_m.last_error(), small_m.last_error()
    print("worst |delta| / bound:", check_rows(got, want, data, scales, x, M, N, K))


@pytest.mark.parametrize("M,in_off,in_rs", [(3, 4, 4096 + 8), (5, 5, 4096 + 7)])  # (the second: rows not 8-byte aligned, scalar x loads)
def test_rows_kernel_offsets_and_strides(small_m, oracle, M, in_off, in_rs):
    K, N = 4096, 4096
    x, data, scales = q4_case(0x51D + M, M, K, N)
    want, got = run_both(small_m, oracle, data, scales, x, M, N, K, in_off=in_off, in_rs=in_rs, dst_off=3, dst_rs=N + 5)
    assert not small_m.last_error(), small_m.last_error()
    check_rows(got, want, data, scales, x, M, N, K, dst_off=3, dst_rs=N + 5)


@pytest.mark.parametrize("M", [2, 8])
def test_all_eight_nibbles_give_exact_zeros(small_m, oracle, M):
    """Every stored nibble 8 (weight value 0): the per-row offset term cancels the accumulation chain term by term, as in the M = 1
    kernel (kon_fold_wave), so every output is exactly 0 — not merely small."""
    K, N = 4096, 4096
    x, _, scales = q4_case(0x0E16 + M, M, K, N)
    data = np.zeros(K * N, np.int8)
    prog, _ = program(data, scales, x, M, N, K)
    assert ROWS_TAG in plan_of(small_m, prog)
    want, got = run_both(small_m, oracle, data, scales, x, M, N, K)
    assert np.all(want[:M * N] == 0) and np.all(got[:M * N] == 0) and np.all(got[M * N:] == -7)
    assert not np.any(np.signbit(got[:M * N]) & (got[:M * N] != 0))


@pytest.mark.parametrize("M", [2, 4, 8])
def test_option_off_keeps_the_tile_kernels(hip_backend, oracle, M):
    K, N = 4096, 4096
    x, data, scales = q4_case(0x0FF + M, M, K, N)
    prog, _ = program(data, scales, x, M, N, K)
    assert ROWS_TAG not in plan_of(hip_backend, prog)
    want, got = run_both(hip_backend, oracle, data, scales, x, M, N, K)
    assert not hip_backend.last_error(), hip_backend.last_error()
    check_rows(got, want, data, scales, x, M, N, K)


def test_default_bound_routes_six_rows_and_refuses_a_refresh_to_seven(hip_backend, oracle):
    """Option value 1: M <= 6 over the new kernel; an M = 7 op keeps the tile kernels, and raising a packed weight's M to 7 is refused."""
    K, N = 4096, 64
    x, data, scales = q4_case(0x61, 7, K, N)
    hip_backend.set_option(capi.OPT_SMALL_M_MATVEC, 1)
    try:
        assert ROWS_TAG in plan_of(hip_backend, program(data, scales, x[:6 * K], 6, N, K)[0])
        assert ROWS_TAG not in plan_of(hip_backend, program(data, scales, x, 7, N, K)[0])
        want, got = run_both(hip_backend, oracle, data, scales, x, 7, N, K)
        check_rows(got, want, data, scales, x, 7, N, K)
        h = hip_backend.compileProgram(program(data, scales, x[:6 * K], 6, N, K)[0])
    finally:
        hip_backend.set_option(capi.OPT_SMALL_M_MATVEC, 0)
    assert h, hip_backend.last_error()
    try:
        hip_backend.refreshProgram(h, [DeviceOp.qmatmul(1, 0, 0, 7, N, K)])
        err = hip_backend.last_error()
        assert "refresh_program" in err and "M <= 6" in err and "recompile" in err, err
        capi.load_hip().zgml_hip_clear_error(hip_backend.ctx)
    finally:
        hip_backend.freeProgram(h)


def test_short_k_keeps_the_n_on_lanes_layout(small_m, oracle):
    """K below the K-on-lanes threshold (SmolLM's 576): the option changes nothing, 2 <= M <= 8 stays on the tile kernels."""
    M, K, N = 4, 576, 1536
    x, data, scales = q4_case(0x576, M, K, N)
    prog, _ = program(data, scales, x, M, N, K)
    assert ROWS_TAG not in plan_of(small_m, prog)
    want, got = run_both(small_m, oracle, data, scales, x, M, N, K)
    check_rows(got, want, data, scales, x, M, N, K)


def test_refresh_to_nine_rows_over_a_weight_packed_for_eight_is_refused(small_m, oracle):
    K, N = 4096, 64
    x, data, scales = q4_case(0x9, 9, K, N)
    prog, dst_len = program(data, scales, x, 9, N, K)
    op8 = DeviceOp.qmatmul(1, 0, 0, 8, N, K)
    prog8 = DeviceProgram(ops=[op8], buffer_sizes=prog.buffer_sizes, initial_uploads=prog.initial_uploads, qweights=prog.qweights)
    want = oracle.run_program(prog8, 1, dst_len)
    h = small_m.compileProgram(prog8)
    assert h, small_m.last_error()
    try:
        assert ROWS_TAG in small_m.planText(h)
        out = np.zeros(dst_len, f32)
        small_m.executeProgram(h, [], [ProgramIO(1, out)])
        assert not small_m.last_error(), small_m.last_error()
        small_m.refreshProgram(h, [DeviceOp.qmatmul(1, 0, 0, 9, N, K)])
        err = small_m.last_error()
        assert "refresh_program" in err and "M <= 8" in err and "recompile" in err, err
        capi.load_hip().zgml_hip_clear_error(small_m.ctx)
        out2 = np.full(dst_len, 5, f32)
        small_m.executeProgram(h, [], [ProgramIO(1, out2)])  # the previous (M = 8) ops are still in force
        assert not small_m.last_error(), small_m.last_error()
        assert np.array_equal(out2, out)
        bb = bound(data, scales, x[:8 * K], 8, N, K, 32)
        assert np.all(np.abs(out[:8 * N].astype(np.float64) - want[:8 * N]) <= TOL * bb.ravel() + 1e-30)
    finally:
        small_m.freeProgram(h)
