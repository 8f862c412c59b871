"""The refresh contract (zgml_hip_refresh_program, VTable.refresh_program): after a refresh that changes a STATIC field of an op,
the next execute must compute what the reference's CPU backend computes — it re-reads every op on every execute. Each case
compiles a small program, executes it, refreshes one field and executes again on both backends; every buffer is compared
after each execute. Among them the stores with patch_stride == 0, whose offset / column is static: a moved dst_offset or col
must reach the plan (it used to be dropped as if it were the per-token dynamic field)."""
import numpy as np
import pytest

from zgml_amd import DeviceOp, DeviceProgram, FusedEwStep, MatMulGeometry, ProgramIO, QuantizedWeightUpload, capi

pytestmark = pytest.mark.gpu
f32 = np.float32


def check_refresh(be, oracle, prog, refreshes, atol=2e-5):
    ref = oracle.OracleBackend()
    hr = ref.compileProgram(prog)
    be.set_option(capi.OPT_SKIP_DEAD_UPLOADS, 0)  # every buffer stays readable, also one a refresh stops referencing
    try:
        h = be.compileProgram(prog)
    finally:
        be.set_option(capi.OPT_SKIP_DEAD_UPLOADS, 1)
    assert h, be.last_error()
    try:
        for step, ops in enumerate([None] + list(refreshes)):
            if ops is not None:
                be.refreshProgram(h, ops)
                ref.refreshProgram(hr, ops)
            outs = [ProgramIO(b, np.zeros(int(s), f32)) for b, s in enumerate(prog.buffer_sizes)]
            be.executeProgram(h, [], outs)
            ref.executeProgram(hr, [], [])
            assert not be.last_error(), be.last_error()
            for b, io in enumerate(outs):
                want = ref.buffer(hr, b)
                scale = max(1.0, float(np.abs(want).max()))
                np.testing.assert_allclose(io.host, want, rtol=0, atol=atol * scale, err_msg=f"step {step}, buffer {b}")
    finally:
        be.freeProgram(h)
        ref.freeProgram(hr)


def _ups(rng, sizes, lo=-1.0, hi=1.0):
    return [ProgramIO(b, rng.uniform(lo, hi, s).astype(f32)) for b, s in enumerate(sizes)]


@pytest.mark.parametrize("moves", [[8], [8, 0, 20]])
def test_static_slice_assign_moved_dst_offset(hip_backend, oracle, moves):
    """slice_assign with patch_stride == 0: refresh to another dst_offset (and back)"""
    rng = np.random.default_rng(10)
    op = DeviceOp.slice_assign(1, 0, 4, 2, 0, 0, 1, 4, 0, 1, 4, 0)
    sizes = [8, 32]
    check_refresh(hip_backend, oracle, DeviceProgram([op], sizes, _ups(rng, sizes)), [[op.with_(dst_offset=d)] for d in moves])


def test_static_slice_assign_moved_behind_an_attention(hip_backend, oracle):
    """the same store folded into the attention that produces its rows (the row store of a head)"""
    rng = np.random.default_rng(11)
    dh, skv = 8, 5
    att = DeviceOp.attention(4, 0, 1, 2, 3, False, dh, 1, skv, 0.35, 0, 0, 0, 0, 0, 1, dh, 1, dh, 1, dh, 1, 1, 1, dh)
    row = DeviceOp.slice_assign(5, 4, dh, 1, 0, 0, 1, dh, 0, 1, dh, 0)
    sizes = [dh, dh * skv, dh * skv, 1, dh, 4 * dh]
    prog = DeviceProgram([att, row], sizes, _ups(rng, sizes))
    check_refresh(hip_backend, oracle, prog, [[att, row.with_(dst_offset=2 * dh)], [att, row.with_(dst_offset=dh)]])


def test_static_kvq_store_moved_col(hip_backend, oracle):
    """kvq_store with patch_stride == 0: refresh to another column; the attention over the cache reads it"""
    rng = np.random.default_rng(12)
    dh, n_cols = 32, 4
    cache = n_cols * dh // 4 + n_cols * (dh // 32)
    st = DeviceOp.kvq_store(0, 2, dh, 32, n_cols, 0, 0, 0, 0)
    sv = DeviceOp.kvq_store(1, 3, dh, 32, n_cols, 0, 0, 0, 0)
    att = DeviceOp.attention_kvq(5, 4, 0, 1, 0, False, dh, 1, n_cols, 0.2, 32, n_cols, 0, 0, 0, dh, 0, dh)
    sizes = [cache, cache, dh, dh, dh, dh]
    ups = [ProgramIO(0, np.zeros(cache, f32)), ProgramIO(1, np.zeros(cache, f32))] + _ups(rng, sizes)[2:]
    prog = DeviceProgram([st, sv, att], sizes, ups)
    check_refresh(hip_backend, oracle, prog, [[st.with_(col=2), sv.with_(col=2), att], [st.with_(col=3), sv, att]], atol=3e-4)


def test_static_fields_of_every_kind(hip_backend, oracle):
    """one program of the elementwise, row, rope, attention, reduce and repeat kinds; each refresh changes one static field"""
    rng = np.random.default_rng(13)
    n, dh = 64, 8
    # 0 x, 1 y, 2 e, 3 f, 4 rows, 5 cs, 6 rope, 7 att, 8 red, 9 rep
    sizes = [n, n, n, n, n, 4 * dh, 2 * dh, dh, 8, 3 * dh]
    ops = [DeviceOp.elementwise("add", 2, 0, 1, 48, 0, 4, 8),
           DeviceOp.fused_elementwise([FusedEwStep("mul", False, 1, 0), FusedEwStep("neg")], 32, 3, 2, 0, 0),
           DeviceOp.rmsnorm(4, 3, 2, 16, 1e-5),
           DeviceOp.rope(6, 0, 5, dh // 2, 2, 0, 0, 0, 1, dh, 2 * dh),
           DeviceOp.attention(7, 6, 0, 1, 4, True, dh, 1, 4, 0.3, 0, 0, 8, 0, 0, 1, dh, 1, dh, 1, dh, 1, 4, 1, dh),
           DeviceOp.reduce("sum", 8, 4, 4, 8),
           DeviceOp.repeat(9, 7, 3 * dh, (dh, 1, 1, 1), (dh, 3, 1, 1), (1, dh, dh, dh), (1, dh, 3 * dh, 3 * dh)),
           DeviceOp.softmax(1, 9, 2, 12, dst_offset=40)]
    changes = [(0, dict(op="mul")), (0, dict(src1_offset=12)), (0, dict(dst=3)), (0, dict(n=40)),
               (1, dict(steps=[FusedEwStep("add", True, 1, 4), FusedEwStep("abs")])),
               (2, dict(eps=0.5)), (2, dict(rows=1, cols=32)), (2, dict(src_offset=8)),
               (3, dict(src_off=dh)), (4, dict(scale=1.1)), (4, dict(has_mask=False)), (4, dict(mask_off=2)),
               (5, dict(op="max")), (6, dict(src=6)), (7, dict(cols=6, rows=4))]
    refreshes = []
    for i, ch in changes:
        cur = list(ops)
        cur[i] = ops[i].with_(**ch)
        refreshes.append(cur)
    check_refresh(hip_backend, oracle, DeviceProgram(ops, sizes, _ups(rng, sizes, 0.1, 1.0)), refreshes)


def test_static_fields_of_matmuls_and_layernorm(hip_backend, oracle):
    """dense matmul, M = 1 and M > 1 qmatmuls with row strides, layernorm: each refresh changes one offset, stride, weight or
    eps (the qmatmul is the anchor of most fused launches: its M = 1 form carries the rmsnorm prologue and an add epilogue)"""
    rng = np.random.default_rng(14)
    K, N, M = 64, 32, 3
    # 0 x rows, 1 gamma, 2 xn (norm), 3 xg, 4 y, 5 r, 6 z, 7 Y rows, 8 a, 9 b, 10 c, 11 ln
    sizes = [M * (K + 8), K, K + 8, K + 8, N + 8, N, N + 8, M * (N + 8), 24, 24, 24, 64]
    w = [QuantizedWeightUpload(rng.integers(-8, 8, K * N).astype(np.int8), (rng.random(K * N // 32) * 0.05 + 0.01).astype(f32), K, N, 32)
         for _ in range(2)]
    ops = [DeviceOp.rmsnorm(2, 0, 1, K, 1e-5),
           DeviceOp.elementwise("mul", 3, 2, 1, K),
           DeviceOp.qmatmul(4, 3, 0, 1, N, K),
           DeviceOp.elementwise("add", 6, 4, 5, N),
           DeviceOp.qmatmul(7, 0, 1, M, N, K, input_row_stride=K + 8, dst_row_stride=N + 8),
           DeviceOp.matmul(10, 8, 9, MatMulGeometry(2, 3, 4, 4, 1, 3, 1, 0, 0, 0, 3)),
           DeviceOp.layernorm(11, 0, 2, 16, 1e-5)]
    changes = [(2, dict(input_offset=4)), (2, dict(dst_offset=8)), (2, dict(weight_idx=1)), (3, dict(src1_offset=0, dst_offset=4)),
               (4, dict(input_row_stride=K + 4)), (4, dict(dst_row_stride=N + 4, dst_offset=4)), (4, dict(input_offset=8)),
               (5, dict(geom=MatMulGeometry(2, 3, 4, 1, 2, 1, 4, 1, 2, 4, 5))), (6, dict(eps=0.25)), (6, dict(src_offset=8, rows=3))]
    refreshes = []
    for i, ch in changes:
        cur = list(ops)
        cur[i] = ops[i].with_(**ch)
        refreshes.append(cur)
    check_refresh(hip_backend, oracle, DeviceProgram(ops, sizes, _ups(rng, sizes), qweights=w), refreshes, atol=1e-4)
