"""The f16-promoted dense matmul (zgml_amd/csrc/dense_f16.hip) on the device, through the case table of tests/dense_f16_cases.py
(pinned on the CPU by tests/test_dense_f16_cases_host.py): every instantiation default switches reach, at the cuts of its loop,
against float64 over the operands as the kernel rounds them, |got - want| <= 2e-5 * (|a'| @ |b'|) + 1e-30 on every output.
(An output of an M > 1 form on the f16_edges profile that misses it is held to the contract plus 2^-14 * |other operand| per
subnormal operand of its 32-k dots that mix magnitudes by 2^15 or more, never in a subnormal-only column and for at most 64
outputs of a matmul: what the matrix instruction was measured to need; dense_f16_cases.py says why. The PARITY lines also give
every case's worst error over the contract alone.)
Per case: no error, the launches the restated planner expects in the plan text, every word outside the outputs untouched, a
second execution bit-equal to the first. Bit-equal properties: a row does not depend on the other rows of its launch; a part of
a grouped launch, a launch that reuses the packed A, and every launch of the non-temporal (NT) program equal the same matmul in
a program of its own. A refused promotion is bit-equal to the program with the option off.

The switches ZGML_F16_TILE2, ZGML_F16_TILE2_CG, ZGML_F16_TILE2_WIDE and ZGML_F16_TILE2_WAVES are latched per process: the staged
M > 1 form, the CG = 4 tile kernels and the narrow three-wave R = 2 form run their own tables in a child pytest each.
Not covered: the NT instantiations of those env-only kernels."""
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from zgml_amd import capi
from tests import dense_f16_cases as DF

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FORCED_KEY = next((k for k, env in DF.FORCED.items() if all(os.environ.get(n) == str(v) for n, v in env.items())), None)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture()
def f16_on(hip_backend):
    hip_backend.set_option(capi.OPT_F16_DENSE_WEIGHTS, 1)
    yield hip_backend
    hip_backend.set_option(capi.OPT_F16_DENSE_WEIGHTS, 0)


def launches_of(text):
    return [(int(lo), int(hi)) for lo, hi in re.findall(r"ops \d+ \[(\d+)\.\.(\d+)\]", text)]


def check_case(be, name):
    c = DF.build_case(name)
    assert be.supportsProgram(c.prog)
    bufs = sorted({m.d_buf for m in c.mats} | {b for b, _ in c.zero_ops})
    got, text = DF.run(be, c.prog, bufs, c.exec_inputs, c.images, executes=2, plan_text=True)
    assert not be.last_error(), be.last_error()
    assert launches_of(text) == c.launches, text
    worst, worst_op, of_contract = 0.0, None, 0.0
    for m in c.mats:
        r, alone = DF.check_mat(c, m, got[m.d_buf][0], matrix_cores=True)
        of_contract = max(of_contract, alone)
        if r >= worst:
            worst, worst_op = r, m.op
    first = {b: got[b][0] for b in bufs}
    DF.untouched(c, first)
    for b in bufs:
        assert np.array_equal(bits(got[b][0]), bits(got[b][1])), f"{name}: buffer {b} differs between two executions"
    for b, n in c.zero_ops:
        assert np.all(first[b][:n] == 0), f"{name}: {np.count_nonzero(first[b][:n])} outputs of the zero weight are not zero"
    for i, j, rows in c.same_rows:
        x, y = c.mats[i], c.mats[j]
        assert np.array_equal(bits(first[x.d_buf][x.written()[:rows]]), bits(first[y.d_buf][y.written()[:rows]])), f"{name}: rows depend on the launch's other rows"
    note = ""
    if c.solo_equal:
        for L in DF.plan(c.prog, c.env):
            for op in L.parts:
                m = next((m for m in c.mats if m.op == op), None)
                if m is None:
                    continue
                prog, d = DF.solo_program(c, m)
                alone, _ = DF.run(be, prog, [d])
                same = np.array_equal(bits(first[m.d_buf][m.written()]), bits(alone[d][0][m.written()]))
                solo_cg = DF.route(m.M, m.K, m.N, m.a_off % 4 == 0, m.a_rs, False, c.env).CG
                if solo_cg == c.routes[L.lo].CG:
                    assert same, f"{name}: op {op} differs from the same matmul launched alone"
                else:
                    note += f"; op {op} against the launch alone at CG {solo_cg}: {'bit-equal' if same else 'differs'}"
    if not c.mats[0].promoted:  # the refusal: what runs is the f32 matmul, bit for bit
        be.set_option(capi.OPT_F16_DENSE_WEIGHTS, 0)
        try:
            plain, _ = DF.run(be, c.prog, bufs, c.exec_inputs, c.images)
        finally:
            be.set_option(capi.OPT_F16_DENSE_WEIGHTS, 1)
        for b in sorted({m.d_buf for m in c.mats if not m.promoted}):
            assert np.array_equal(bits(first[b]), bits(plain[b][0])), f"{name}: differs from the program compiled without the promotion"
    print(f"PARITY {name}: worst error / bound = {worst:.3g} at op {worst_op} (bar {DF.TOL:g}, margin {DF.TOL / max(worst, 1e-30):.1f}x; "
          f"{of_contract:.3g} of the contract alone){note}")


@pytest.mark.parametrize("name", DF.DEFAULT_CASES)
def test_case(f16_on, name):
    check_case(f16_on, name)


if FORCED_KEY:  # (the child of test_forced_switches: the process has the switches latched)
    @pytest.mark.parametrize("name", DF.forced_cases(FORCED_KEY))
    def test_forced_case(f16_on, name):
        check_case(f16_on, name)


@pytest.mark.parametrize("key", sorted(DF.FORCED))
def test_forced_switches(key):
    """the env-only kernels over their own tables, the same checks in a process of their own"""
    ids = [f"{Path(__file__)}::test_forced_case[{n}]" for n in DF.forced_cases(key)]
    assert ids
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-s", *ids], capture_output=True, text=True, timeout=300,
                       cwd=ROOT, env=dict(os.environ, **{n: str(v) for n, v in DF.FORCED[key].items()}))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert f"{len(ids)} passed" in r.stdout, r.stdout[-2000:]
    print("".join(ln[ln.index("PARITY"):] + "\n" for ln in r.stdout.splitlines() if "PARITY " in ln), end="")
