"""The hand-off INSIDE the fused q / k / v + decode attention launches (qkv_attn_kernel, qkv_attn_kon_kernel): the projection's 16
owning lanes store {value, generation} granules, one wave of every attention workgroup sweeps its head's granules until every
tag carries the execution's generation (zgml_amd/csrc/handoff_gen.h, qmatvec.hip reduce_store, attention_decode.h). Nothing is
zeroed between executions: producer and consumer generations run on across vtable steps, graph replays and calls. The
K-on-lanes launch ("l7") keeps the counter form of the same hand-off (handoff_gen.h CounterHandoff) and
is held to the same properties here.

Reduced models of tests/test_hip_fused_qkv.py (2 layers, vocabulary 2048, max_seq 256) with the split threshold at 32 keys, so
that from position 64 on several workgroups per head sweep the same granules (GQA: three or four heads per k / v slice anyway).
The bounds between the fused and the refused plan are that file's: 2e-5 of the logit range with f32 KV (the two plans compute
the same sums in the same order; the bound leaves room for nothing but that), its int8 bounds with int8 KV."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from zgml_amd import capi, llama

ROOT = Path(__file__).resolve().parent.parent
PROBE_SRC = ROOT / "tests" / "cpp" / "handoff_gen_probe.cpp"
HEADER = ROOT / "zgml_amd" / "csrc" / "handoff_gen.h"
BUILD = ROOT / "tests" / "cpp" / "_build"

fused_switch_on = pytest.mark.skipif(os.environ.get("ZGML_HIP_FUSE_QKV_ATTN") == "0", reason="the diagnostic switch under test turns the fused launch off")
VARIANTS = [(name, kvq) for name in ("smollm", "dh128", "l7") for kvq in (0, 32)]
N = 80


def _cfg(name, kvq):
    if name == "smollm":  # d 576, 9 x 64, 3 kv heads -> qkv_attn_kernel<..., 16, ...>
        cfg = llama.preset("smollm-135m", 256)
    elif name == "l7":  # Llama-2-7B's layer, K-on-lanes weights -> qkv_attn_kon_kernel<32, ...> (256-thread workgroups, counters)
        cfg = llama.preset("llama2-7b", 256)
    else:  # d 2048, 16 x 128, 4 kv heads -> qkv_attn_kernel<..., 32, ...>
        cfg = llama.preset("smollm-135m", 256)
        cfg.d_model, cfg.n_heads, cfg.n_kv_heads, cfg.d_ff = 2048, 16, 4, 2048
    cfg.n_layers, cfg.vocab_size, cfg.kv_quant_block = 2, 2048, kvq
    return cfg


_models, _fused_runs = {}, {}


def _model(name, kvq):
    if (name, kvq) not in _models:
        _models[name, kvq] = llama.Model(_cfg(name, kvq), llama.Q4_0, threads=8)
    return _models[name, kvq]


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _models.values():
        m.close()
    _models.clear(), _fused_runs.clear()


@pytest.fixture
def split32(hip_backend):
    hip_backend.set_option(capi.OPT_ATTN_SPLIT_MIN_KEYS, 32)
    yield hip_backend
    hip_backend.set_option(capi.OPT_FUSE_RESIDENT_WGS, -1)
    hip_backend.set_option(capi.OPT_ATTN_SPLIT_MIN_KEYS, -1)


def _dispatches(be, s):
    return capi.load_hip().zgml_hip_get_runtime_profile(be.ctx, s.handle).contents.backend_dispatch_count


def _run(be, m, tokens=None):
    """N greedy vtable steps of a fresh session from token 3 (fed `tokens` instead of its own picks when given)
    -> (picks, logits [N, vocab], launches per step)"""
    s = llama.Session(m, llama.hip_backend_fns(be))
    tok, picks, logits = 3, [], []
    for pos in range(N):
        t, l = s.step(tok, pos)
        assert not be.last_error(), (pos, be.last_error())
        picks.append(t), logits.append(l)
        tok = t if tokens is None else tokens[pos]
    launches = _dispatches(be, s) // N
    s.close()
    return picks, np.stack(logits), launches


def _fused_run(be, name, kvq):
    """the fused program's run, computed once per variant and shared (never modified)"""
    if (name, kvq) not in _fused_runs:
        _fused_runs[name, kvq] = _run(be, _model(name, kvq))
    return _fused_runs[name, kvq]


@fused_switch_on
@pytest.mark.gpu
@pytest.mark.parametrize("name,kvq", VARIANTS)
def test_fused_against_refused(split32, name, kvq):
    """80 vtable steps through the fused launch, then the same tokens through the plan with the fusion refused (one launch more per
    fused layer): logits within 2e-5 of the range (int8 KV: tests/test_hip_fused_qkv.py's bounds), equal picks, no error."""
    be = split32
    picks, logits, launches = _fused_run(be, name, kvq)
    assert np.isfinite(logits).all()
    be.set_option(capi.OPT_FUSE_RESIDENT_WGS, 0)
    picks_u, logits_u, launches_u = _run(be, _model(name, kvq), tokens=picks)
    tol = ((6e-3 if name == "l7" else 1e-3) if kvq else 2e-5)
    err = (np.abs(logits_u - logits).max(axis=1) / np.abs(logits).max(axis=1)).max()
    print(f"{name} kvq={kvq}: fused against refused, worst |diff| / range = {err:.3g} (bound {tol:g}); launches {launches} / {launches_u}")
    assert err < tol
    assert picks_u == picks
    # (K-on-lanes models: the first layer's q / k / v launch computes its rmsnorm itself and stays apart; the diagnostic switches
    # that take away the layout, the prepared norm or this fusion leave nothing to refuse)
    kon_off = any(os.environ.get(v) == "0" for v in ("ZGML_HIP_FUSE_QKV_ATTN_KON", "ZGML_HIP_QMV_KON", "ZGML_HIP_PRENORM"))
    more = (0 if kon_off else 1) if name == "l7" else 2
    assert launches_u == launches + more, "the fused launch under test was not built"


@fused_switch_on
@pytest.mark.gpu
@pytest.mark.parametrize("name,kvq", VARIANTS)
def test_two_fresh_sessions_give_equal_bits(split32, name, kvq):
    """Arrival order of the granules must not show: a second fresh session of the fused program repeats the first one's logits
    bit for bit at every position."""
    be = split32
    picks, logits, _ = _fused_run(be, name, kvq)
    picks2, logits2, _ = _run(be, _model(name, kvq))
    assert picks2 == picks
    assert np.array_equal(logits2, logits)


@fused_switch_on
@pytest.mark.gpu
@pytest.mark.parametrize("name,kvq", VARIANTS)
def test_generations_run_on_under_graph_replay(split32, name, kvq):
    """Three calls of the resident loop over positions 0..199 on one session: 600 graph replays, every word of the hand-off state
    carried from replay to replay and from call to call, with the vtable path's executions of the same launches in between. Each
    call gives the vtable path's tokens and no wait times out."""
    be = split32
    s = llama.Session(_model(name, kvq), llama.hip_backend_fns(be))
    try:
        s.resident_setup(be)
        for call in range(3):
            got = s.resident_decode(3, 0, 200)  # (raises on a time-out: the call returns -1)
            assert not be.last_error(), (call, be.last_error())
            want, _ = s.decode(3, 0, 200)
            assert not be.last_error(), (call, be.last_error())
            assert got.tolist() == want.tolist(), call
    finally:
        s.close()


def test_generation_rule_on_the_cpu():
    """handoff_gen.h without a GPU: next(g) is never 0, next(0xFFFFFFFF) == 1 (static assertions in the probe as well), and a
    producer word and a consumer word that both start at 0 stay equal over the wrap, never waiting for a stale or zeroed tag."""
    exe = BUILD / "handoff_gen_probe"
    BUILD.mkdir(parents=True, exist_ok=True)
    if not exe.exists() or any(p.stat().st_mtime > exe.stat().st_mtime for p in (PROBE_SRC, HEADER)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", str(exe), str(PROBE_SRC)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = dict(kv.split("=") for kv in r.stdout.split())
    assert out["ok"] == "1" and out["zeros"] == "0" and out["unequal"] == "0" and out["stale_match"] == "0"
    assert out["next_of_max"] == "1" and out["next_of_zero"] == "1"
    assert int(out["steps"]) == (1 << 20) + (1 << 21)
