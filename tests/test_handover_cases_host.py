"""The case table of tests/handover_cases.py on the oracle: every program runs, and the oracle's X and Y lie inside the bars the
device test uses against the table's float64 references. That shows the inputs keep the references themselves well inside the
bars (what the device then misses is the device's), and that the near misses' expected values include the writer between producer
and consumer: a reference that ignored it fails here."""
import numpy as np
import pytest

from tests import handover_cases as HC


def run_steps(oracle, c):
    """[{buffer: f32 copy} per step] on the oracle"""
    oracle.set_f16_dense(c.f16)
    try:
        be = oracle.OracleBackend()
        h = be.compileProgram(c.prog)
    finally:
        oracle.set_f16_dense(False)
    assert h
    try:
        out = []
        for st in c.steps:
            if st.ops is not None:
                be.refreshProgram(h, st.ops)
            be.executeProgram(h, [], [])
            out.append({b: be.buffer(h, b).copy() for b in range(len(c.prog.buffer_sizes))})
        return out
    finally:
        be.freeProgram(h)


def check_step(c, st, bufs, what):
    """X against the float64 producer reference, every Y against the float64 consumer reference of the X really produced, the
    sentinels behind every Y. Returns the largest |delta| / bound per consumer kind."""
    rows, cols = st.x_ref.shape
    x = bufs[c.x_buf][c.x_off:][:rows * cols].reshape(rows, cols)
    err = float(np.abs(x - st.x_ref).max())
    print(f"{what}: max |X - ref| = {err:.3g}")
    np.testing.assert_allclose(x, st.x_ref, err_msg=f"{what}: X", **c.bars)
    worst = {}
    for k, co in enumerate(st.consumers):
        want, bound = co.reference(co.x(bufs))
        y = bufs[co.y_buf]
        got = y[:co.M * co.N].reshape(co.M, co.N)
        ratio = np.abs(got - want) / (bound + 1e-300)
        m = int(np.argmax(ratio.max(axis=1)))
        print(f"{what}: consumer {k} ({co.kind}, M {co.M} K {co.K} N {co.N}) max |Y - ref| / bound = {ratio.max():.3g} (row {m})")
        worst[co.kind] = max(worst.get(co.kind, 0.0), float(ratio.max()))
        assert np.all(np.abs(got - want) <= HC.TOL * bound + 1e-30), f"{what}: consumer {k} row {m} off by {ratio.max():.3g} of its bound"
        assert np.all(y[co.M * co.N:] == HC.SENTINEL), f"{what}: consumer {k} wrote behind its {co.M} rows"
    return worst


@pytest.mark.parametrize("name", HC.CASE_NAMES)
def test_oracle_inside_the_bars(oracle, name):
    c = HC.build_case(name)
    for k, (st, bufs) in enumerate(zip(c.steps, run_steps(oracle, c))):
        check_step(c, st, bufs, f"{name} step {k}")


@pytest.mark.parametrize("name", [n for n in HC.CASE_NAMES if n.startswith("writer_")])
def test_writer_changes_the_expected_rows(oracle, name):
    """the near misses are near misses: the producer's own output, without the writer, is outside the bars of the expected X"""
    c = HC.build_case(name)
    st = c.steps[0]
    chain_only = HC.DeviceProgram(ops=c.prog.ops[:2],  # the case's own [rmsnorm -> mul]
                                   buffer_sizes=c.prog.buffer_sizes, initial_uploads=c.prog.initial_uploads)
    x = oracle.run_program(chain_only, c.x_buf, c.prog.buffer_sizes[c.x_buf])[:st.x_ref.size].reshape(st.x_ref.shape)
    assert not np.allclose(x, st.x_ref, **c.bars)


def test_table_shape():
    """the table keeps the outcomes it is there for: the producer forms that must be armed, the shapes that must not be, and no near miss
    (static refreshes apart, whose tag comes and goes) that expects an armed launch"""
    assert len(HC.CASE_NAMES) == len(set(HC.CASE_NAMES))
    for n in HC.CONTROL_NAMES:
        assert HC.build_case(n).control, n
    armed = [n for n in HC.CONTROL_NAMES if HC.build_case(n).steps[0].tagged]
    for must in ("row_16x128_q4", "row_16x8320_f16", "row_80x256_q4", "row_16x96_f16", "elt_128x8192_q4", "elt_refactored_f16", "attn_64x3_q16_f16",
                 "group_qkv_q4", "stale_scratch_q4"):
        assert must in armed, must
    for never in ("row_80x256_f16", "row_16x96_q4", "row_16x288_q4", "row_32x160_q4", "elt_16x96_q4", "attn_64x3_q16_q4"):
        assert HC.build_case(never).steps[0].tagged == set(), never
    for n in HC.CASE_NAMES:
        if n not in HC.CONTROL_NAMES:
            assert n.startswith("refresh_") or all(st.tagged == set() for st in HC.build_case(n).steps), n
