"""Every case of tests/generic_cases.py on the device: each compared buffer against the float64 reference under the a-priori bounds
stated there (equal bits with numpy float32 for the exactly rounded elementwise ops, equal bits with the oracle for repeat, rope
and slice_assign and where a case says so), the fused launches on the plan text, and sentinels untouched to the bit. Every route
is reached by shape alone. Prints the largest error / bound per case and the largest error in ulps of exp / log / gelu."""
import os
import re

import numpy as np
import pytest

from zgml_amd import ProgramIO
from tests import generic_cases as GC

pytestmark = pytest.mark.gpu
f32 = np.float32
_oracle_runs = {}
_worst = {}  # group -> largest error / bound seen


def launches(text):
    """plan text -> {(kind, n_ops, lo, hi)}"""
    out = set()
    for line in text.splitlines():
        m = re.match(r"\d+: kind (\d+) ops (\d+) \[(\d+)\.\.(\d+)\]", line)
        assert m, line
        out.add(tuple(int(g) for g in m.groups()))
    return out


def oracle_run(oracle, c):
    """[buffers per execute] of the case on the oracle: computed once, shared, never modified"""
    if c.name not in _oracle_runs:
        _oracle_runs[c.name] = GC.run_oracle(oracle.OracleBackend(), c)
    return _oracle_runs[c.name]


def run_device(be, c):
    """([{buffer: array} of the checked buffers per execute], [plan text per execute])"""
    assert be.supportsProgram(c.prog)
    h = be.compileProgram(c.prog)
    assert h, be.last_error()
    try:
        outs, texts = [], []

        def execute(inputs=()):
            ios = [ProgramIO(b, np.zeros(c.prog.buffer_sizes[b], f32)) for b in c.checked_buffers()]
            be.executeProgram(h, list(inputs), ios)
            assert not be.last_error(), be.last_error()
            outs.append({io.buf_idx: io.host for io in ios})
            texts.append(be.planText(h))
        execute()
        for ops in c.refresh:
            be.refreshProgram(h, ops)
            execute()
        if c.inputs:
            execute(c.inputs)
        return outs, texts
    finally:
        be.freeProgram(h)


def check(c, outs, oracle_outs=None):
    worst = 0.0
    for i, bufs in enumerate(outs):
        for ck in c.checks:
            worst = max(worst, GC.hold(ck, bufs, "bound", oracle_bufs=oracle_outs[i] if oracle_outs else None))
        GC.untouched(c, bufs)
    _worst[c.group] = max(_worst.get(c.group, 0.0), worst)
    print(f"{c.name}: max error / bound = {worst:.3g} ({c.group} so far: {_worst[c.group]:.3g})")
    return worst


def run_case(be, oracle, name):
    c = GC.build_case(name)
    outs, texts = run_device(be, c)
    seen = launches(texts[0])
    for launch in c.launches:
        assert launch in seen, f"{name}: no launch {launch} in\n{texts[0]}"
    needs_oracle = any(ck.mode == "oracle" for ck in c.checks)
    check(c, outs, oracle_run(oracle, c) if needs_oracle else None)
    return c, outs, texts


@pytest.mark.parametrize("name", GC.names_of("rows"))
def test_rows(hip_backend, oracle, name):
    run_case(hip_backend, oracle, name)


@pytest.mark.parametrize("cols", GC.NOSPLIT_COLS)
def test_split_rows_equal_unsplit_rows(hip_backend, cols):
    """row_chain_kernel: every workgroup of a row forms the same sum in the same order, so a row comes out with the same bits
    whether 4 / 16 / 32 workgroups share its stores or one does them all"""
    big = GC.nosplit_case(cols)
    small = big.info["small"]
    (sbufs,), (stext,) = run_device(hip_backend, small)
    (bufs,), (text,) = run_device(hip_backend, big)
    assert (GC.K_RMS, 3, 0, 2) in launches(stext) and (GC.K_RMS, 3, 0, 2) in launches(text)
    check(big, [bufs])
    for buf, idx, sbuf, sidx in big.info["pairs"]:
        assert GC.same_bits(bufs[buf][idx], sbufs[sbuf][sidx]), f"cols {cols}: buffer {buf} differs between split and unsplit rows"


@pytest.mark.parametrize("name", GC.names_of("softmax") + GC.names_of("layernorm"))
def test_softmax_layernorm(hip_backend, oracle, name):
    run_case(hip_backend, oracle, name)


@pytest.mark.parametrize("name", GC.names_of("reduce"))
def test_reduce(hip_backend, oracle, name):
    run_case(hip_backend, oracle, name)


@pytest.mark.parametrize("name", GC.names_of("dense"))
def test_dense_matmul(hip_backend, oracle, name):
    run_case(hip_backend, oracle, name)


@pytest.mark.parametrize("name", GC.names_of("eltwise"))
def test_elementwise(hip_backend, oracle, name):
    c, outs, _ = run_case(hip_backend, oracle, name)
    if c.info["op"] in ("exp", "log", "gelu"):
        print(f"{name}: max error = {max(GC.ulps(ck, outs[0]) for ck in c.checks):.3g} ulp over all normal results, "
              f"{max(GC.ulps(ck, outs[0], 1e-2) for ck in c.checks):.3g} ulp over |result| >= 0.01")


@pytest.mark.parametrize("name", GC.names_of("chains"))
def test_elementwise_chains(hip_backend, oracle, name):
    c, _, texts = run_case(hip_backend, oracle, name)
    assert len(launches(texts[0])) == len(c.launches), texts[0]  # nothing but the expected launches


def test_repeat_level(hip_backend, oracle):
    """first the sources are uploads only and the repeats run once at plan build; then the host writes one source (the same
    values) and all four run in the plan, as one launch whose grid is sized for the largest"""
    c, _, texts = run_case(hip_backend, oracle, "repeat_level")
    hoisted = os.environ.get("ZGML_HIP_HOIST_REPEAT") != "0"  # (the diagnostic switch keeps them in the plan from the start)
    assert launches(texts[0]) == (set() if hoisted else set(c.launches_after)), texts[0]
    assert launches(texts[1]) == set(c.launches_after), texts[1]


def test_move_level(hip_backend, oracle):
    c, outs, texts = run_case(hip_backend, oracle, "move_level")
    assert len(outs) == len(GC.MOVE_POSITIONS) and all(launches(t) == set(c.launches) for t in texts), texts
