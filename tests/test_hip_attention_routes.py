"""Every kernel route of the attention launch on the device, through the case table of tests/attention_cases.py: the route the
planner tags, parity with the oracle (atol 2e-5, the bar tests/test_hip_conformance.py uses for attention), untouched sentinels,
and the skip rule — non-finite K / V / scale values at keys the reference skips, and an all-NaN query, must not reach any
output. The switches that take a kernel away are latched per process, so those routes run in a child pytest each."""
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from zgml_amd import ProgramIO
from tests import attention_cases as AC

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = Path(__file__).resolve().parent.parent
ATOL = 2e-5
SWITCHED = {"ZGML_HIP_ATTN_ROWS": AC.ROWS_OFF, "ZGML_HIP_ATTN_TILES": AC.TILES_OFF}
_clean = {}


def expected_tag(c):
    for var, table in SWITCHED.items():
        if os.environ.get(var) == "0" and c.name in table:
            return table[c.name]
    return c.tag


def clean_oracle(oracle, name):
    """[[array per output] per seq_kv] of the clean case on the oracle: computed once, shared, never modified"""
    if name not in _clean:
        c = AC.build_case(name)
        _clean[name] = AC.run_case(oracle.OracleBackend(), c, c.refresh)[0]
    return _clean[name]


def run_device(be, c, seq_kvs=(), executes=1):
    """[[array per output] per seq_kv], plan text; with executes > 1 every further execute must repeat the first bit for bit"""
    h = be.compileProgram(c.prog)
    assert h, be.last_error()
    try:
        text = be.planText(h)
        res = []
        for n in (None,) + tuple(seq_kvs):
            if n is not None:
                be.refreshProgram(h, [o.with_(seq_kv=n) if o.kind in ("attention", "attention_kvq") else o for o in c.prog.ops])
            first = None
            for _ in range(executes):
                outs = [ProgramIO(b, np.zeros(c.prog.buffer_sizes[b], f32)) for b in c.outs]
                be.executeProgram(h, [], outs)
                assert not be.last_error(), be.last_error()
                got = [o.host for o in outs]
                if first is None:
                    first = got
                else:
                    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(first, got)), "executes differ"
            res.append(first)
        return res, text
    finally:
        be.freeProgram(h)


def check(got, want, what):
    for b, (g, w) in enumerate(zip(got, want)):
        assert np.isfinite(g).all(), f"{what}: output {b} has {np.count_nonzero(~np.isfinite(g))} non-finite values"
        err = float(np.abs(g - w).max())
        print(f"{what}: output {b} max |device - oracle| = {err:.3g}")
        assert err <= ATOL, f"{what}: output {b} off by {err:.3g}"
        keep = w == AC.SENTINEL  # where the oracle leaves the upload alone
        assert np.array_equal(g[keep], w[keep]), f"{what}: output {b} sentinels overwritten"


@pytest.mark.parametrize("name", AC.CASE_NAMES)
def test_route_and_parity(hip_backend, oracle, name):
    c = AC.build_case(name)
    assert hip_backend.supportsProgram(c.prog)
    want = clean_oracle(oracle, name)
    got, text = run_device(hip_backend, c, c.refresh, executes=2 if c.twice else 1)
    tag = expected_tag(c)
    tagged = [ln for ln in text.splitlines() if tag in ln + " "]
    assert len(tagged) == 1 and not [ln for ln in text.splitlines() if "attention-" in ln and ln not in tagged], text
    if tag.startswith("attention-"):
        assert re.search(rf"ops {len(c.attention_ops())} ", tagged[0]), text  # one launch for the whole level
    for n, g, w in zip((None,) + tuple(c.refresh), got, want):
        check(g, w, f"{name} seq_kv {n or 'as compiled'}")


@pytest.mark.parametrize("variant", AC.VARIANTS)
@pytest.mark.parametrize("name", AC.SKIP_CASES)
def test_skip_variants(hip_backend, oracle, name, variant):
    """device(poisoned) is finite and within the parity bar of oracle(clean) (tests/test_attention_cases_host.py: the oracle's own
    poisoned run is bit-equal to that)"""
    c = AC.build_case(name, variant)
    want = AC.expected_of_variant(c, variant, clean_oracle(oracle, name)[0])
    got, text = run_device(hip_backend, c)
    assert expected_tag(c) in text + " ", text
    check(got[0], want, f"{name} {variant}")
    if variant == "nan_q" and not c.nan_q_zero:  # (expected_of_variant already holds the zeros; this says "exactly")
        for g, op in zip(got[0], c.attention_ops()):
            assert np.all(AC.gather_out(op, g)[AC.NAN_QUERY] == 0)


@pytest.mark.parametrize("switch", sorted(SWITCHED))
def test_switch_routes(switch):
    """the carriers of a kernel with that kernel switched off: tagged with the route they fall to, same parity and skip checks"""
    table = SWITCHED[switch]
    n_tests = len(table) + len(AC.VARIANTS) * len([n for n in AC.SKIP_CASES if n in table])
    ids = [f"{Path(__file__)}::test_route_and_parity[{n}]" for n in table]
    ids += [f"{Path(__file__)}::test_skip_variants[{n}-{v}]" for n in AC.SKIP_CASES if n in table for v in AC.VARIANTS]
    assert len(ids) == n_tests
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-s", *ids],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, **{switch: "0"}))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert f"{n_tests} passed" in r.stdout, r.stdout[-2000:]
