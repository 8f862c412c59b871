"""Random differential programs for the launch planner: seeded programs of the patterns its passes fuse (mat-vec prologues
and epilogues, row chains, elementwise chains, rope -> slice_assign, a decode-attention group) over shared buffers, with
aliasing injected on purpose (tests/plan_cases.py random_fusable_program). Each runs with fusion on (the default) and with
ZGML_HIP_OPT_FUSION = 0, and both must match the oracle in EVERY buffer: 1e-4 of the largest magnitude the buffer holds
(inputs are O(1); a legality bug gives O(1) errors). This catches hazards in patterns no hand-made near miss names."""
import numpy as np
import pytest

from zgml_amd import ProgramIO, capi
from tests.plan_cases import random_fusable_program

pytestmark = pytest.mark.gpu
f32 = np.float32
SEEDS = list(range(36))


def _run_hip(be, prog, fusion):
    be.set_option(capi.OPT_FUSION, fusion)
    be.set_option(capi.OPT_SKIP_DEAD_UPLOADS, 0)  # every buffer stays readable
    try:
        h = be.compileProgram(prog)
    finally:
        be.set_option(capi.OPT_FUSION, 1)
        be.set_option(capi.OPT_SKIP_DEAD_UPLOADS, 1)
    assert h, be.last_error()
    try:
        outs = [ProgramIO(b, np.zeros(int(s), f32)) for b, s in enumerate(prog.buffer_sizes)]
        be.executeProgram(h, [], outs)
        assert not be.last_error(), be.last_error()
        return [o.host for o in outs], be.planText(h)
    finally:
        be.freeProgram(h)


@pytest.mark.parametrize("seed", SEEDS)
def test_fused_and_serial_plans_match_the_oracle(hip_backend, oracle, seed):
    prog = random_fusable_program(seed)
    ref = oracle.OracleBackend()
    hr = ref.compileProgram(prog)
    try:
        ref.executeProgram(hr, [], [])
        want = [ref.buffer(hr, b).copy() for b in range(len(prog.buffer_sizes))]
    finally:
        ref.freeProgram(hr)
    for fusion in (1, 0):
        got, text = _run_hip(hip_backend, prog, fusion)
        for b, (g, w) in enumerate(zip(got, want)):
            scale = max(1.0, float(np.abs(w[np.isfinite(w)]).max(initial=0.0)))
            np.testing.assert_allclose(g, w, rtol=0, atol=1e-4 * scale, err_msg=f"seed {seed}, fusion {fusion}, buffer {b}\n{text}")


def test_random_programs_exercise_the_passes(hip_backend):
    """the generator reaches the fused forms at all: over the seeds, every pass fires somewhere"""
    seen = set()
    for seed in SEEDS:
        _, text = _run_hip(hip_backend, random_fusable_program(seed), 1)
        for tag in ("pro mul", "pro rmsnorm", "decode-attention"):
            if tag in text:
                seen.add(tag)
        for line in text.splitlines():
            kind, n_ops = (int(v) for v in line.split()[2:5:2])
            if n_ops > 1:
                seen.add(kind)
    # 2: mat-vec with an epilogue, 5: row chain, 8: rope + slice fold, 11: elementwise chain
    assert {"pro mul", "pro rmsnorm", "decode-attention", 2, 5, 8, 11} <= seen, seen
