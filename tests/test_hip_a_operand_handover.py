"""The A-operand hand-over on the device, through the case table of tests/handover_cases.py: an M > 1 matmul takes its bf16
pieces (Q4_0 qmatmul) or f16 halves (f16-promoted dense matmul) from the launch that produced its rows — a row chain, an
elementwise chain, the attention tile kernel — when the planner arms that launch (plan.hip make_single, SplitHook). Per case:
  1. the plan text carries "writes-A-operand" on exactly the launches the table names (none with ZGML_HIP_FUSE_SPLIT=0);
  2. X against the float64 producer reference at the bars the project already uses for that producer;
  3. Y against the float64 consumer reference computed from the DOWNLOADED X: |delta| <= 2e-5 * bound (the two-piece split
     alone accounts for 2^-17);
  4. Y bit-equal to a second program that holds only the matmul(s) over the downloaded X and so runs split_a_kernel /
     pack_a_f16_kernel itself: both routes round the same f32 value the same way (split_a_pieces; round-to-nearest-even halves)
     and the tile kernels sum their K slices in slice order, so any difference is a misplaced or missing piece;
  5. a second execution, and one without the captured graph, repeat the bits.
The near misses (a writer between producer and consumer, a matmul over part of the produced rows, static refreshes) must not arm
the stale producer, and their values follow the reference all the same."""
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from zgml_amd import ProgramIO, capi
from tests import handover_cases as HC
from tests.test_handover_cases_host import check_step

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = Path(__file__).resolve().parent.parent
FUSE_OFF = os.environ.get("ZGML_HIP_FUSE_SPLIT") == "0"


def launches(text):
    """plan text -> [(op_lo, op_hi, n_ops, tagged)]"""
    out = []
    for line in text.splitlines():
        m = re.match(r"\d+: kind \d+ ops (\d+) \[(\d+)\.\.(\d+)\](.*)", line)
        assert m, line
        out.append((int(m[2]), int(m[3]), int(m[1]), HC.TAG in m[4]))
    return out


def compile_all_live(be, prog, f16):
    be.set_option(capi.OPT_SKIP_DEAD_UPLOADS, 0)  # every buffer stays readable
    be.set_option(capi.OPT_F16_DENSE_WEIGHTS, int(f16))
    try:
        h = be.compileProgram(prog)
    finally:
        be.set_option(capi.OPT_SKIP_DEAD_UPLOADS, 1)
        be.set_option(capi.OPT_F16_DENSE_WEIGHTS, 0)
    assert h, be.last_error()
    return h


def download(be, h, prog, bufs):
    outs = [ProgramIO(b, np.zeros(prog.buffer_sizes[b], f32)) for b in bufs]
    be.executeProgram(h, [], outs)
    assert not be.last_error(), be.last_error()
    return {io.buf_idx: io.host for io in outs}


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name", HC.CASE_NAMES)
def test_handover(hip_backend, name):
    be, c = hip_backend, HC.build_case(name)
    assert be.supportsProgram(c.prog)
    h = compile_all_live(be, c.prog, c.f16)
    try:
        for k, st in enumerate(c.steps):
            what = f"{name} step {k}"
            if st.ops is not None:
                be.refreshProgram(h, st.ops)
            text = be.planText(h)
            ls = launches(text)
            if st.tagged is not None:
                want = set() if FUSE_OFF else st.tagged
                assert {(lo, hi) for lo, hi, _, t in ls if t} == want, f"{what}: tagged launches, expected {sorted(want)}\n{text}"
            if c.group:
                assert c.group in [(lo, hi, n) for lo, hi, n, _ in ls], f"{what}: no launch of ops {c.group}\n{text}"
            wanted = sorted({c.x_buf, *c.downloads, *(co.x_buf for co in st.consumers), *(co.y_buf for co in st.consumers)})
            bufs = download(be, h, c.prog, wanted)
            check_step(c, st, bufs, what)
            # the matmuls alone over the rows the device produced: they prepare their own A operand
            alone = HC.matmul_only(c, st, bufs)
            ha = compile_all_live(be, alone, c.f16)
            try:
                assert not any(t for *_, t in launches(be.planText(ha)))
                ys = sorted({co.y_buf for co in st.consumers})
                ref = download(be, ha, alone, ys)
            finally:
                be.freeProgram(ha)
            for y in ys:
                diff = np.flatnonzero(bufs[y].view(np.uint32) != ref[y].view(np.uint32))
                assert diff.size == 0, f"{what}: buffer {y} differs from the matmul's own A operand at {diff.size} elements, first {diff[:8]}\n{text}"
            again = download(be, h, c.prog, wanted)
            be.set_option(capi.OPT_GRAPH, 0)
            try:
                eager = download(be, h, c.prog, wanted)
            finally:
                be.set_option(capi.OPT_GRAPH, 1)
            for b in wanted:
                assert same_bits(bufs[b], again[b]), f"{what}: buffer {b} differs in the second execution"
                assert same_bits(bufs[b], eager[b]), f"{what}: buffer {b} differs without the captured graph"
    finally:
        be.freeProgram(h)


def test_controls_with_the_hand_over_switched_off():
    """ZGML_HIP_FUSE_SPLIT=0 (latched per process: a child pytest): no launch is armed, every control holds the same checks"""
    ids = [f"{Path(__file__)}::test_handover[{n}]" for n in HC.CONTROL_NAMES]
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-s", *ids],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, ZGML_HIP_FUSE_SPLIT="0"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert f"{len(ids)} passed" in r.stdout, r.stdout[-2000:]
