"""The wait of the granule hand-off inside qkv_attn_kernel as zgml_amd/csrc/sweep_ring.h states it (a sweep's loads issued
together; one sweep in flight at d_head 64, two at d_head 128: attention_decode.h, profiles/r30_sweep_ring.txt). The wait decides
WHEN a value is read, never which value or the order of any sum, so the fused plan must give the bits of the plan with the
fusion refused wherever both run the same workgroup shape.

Reduced models of tests/test_hip_handoff_granules.py (2 layers, vocabulary 2048, max_seq 256; `smollm`: d_head 64, `dh128`:
d_head 128; f32 and int8 KV). With the split threshold at 32 keys, positions 0..15 run ONE wave (the sweeping wave alone, no
barrier), from 16 on two and more wait behind it, from 64 on two splits per head are live and the idle ones advance their
generation. At the default threshold over positions 0..199 up to 13 waves wait behind the sweeping wave and no split is live: the
headline's regime."""
import os

import numpy as np
import pytest

from zgml_amd import capi, llama

fused_switch_on = pytest.mark.skipif(os.environ.get("ZGML_HIP_FUSE_QKV_ATTN") == "0", reason="the diagnostic switch under test turns the fused launch off")

_models = {}


def _model(name, kvq, own=""):
    """one model per variant; `own` names a further instance of a variant (a model's sessions share ONE compiled program)"""
    if (name, kvq, own) not in _models:
        cfg = llama.preset("smollm-135m", 256)  # d 576, 9 x 64, 3 kv heads -> qkv_attn_kernel<..., 16, ...>
        if name == "dh128":  # d 2048, 16 x 128, 4 kv heads -> qkv_attn_kernel<..., 32, ...>
            cfg.d_model, cfg.n_heads, cfg.n_kv_heads, cfg.d_ff = 2048, 16, 4, 2048
        cfg.n_layers, cfg.vocab_size, cfg.kv_quant_block = 2, 2048, kvq
        _models[name, kvq, own] = llama.Model(cfg, llama.Q4_0, threads=8)
    return _models[name, kvq, own]


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _models.values():
        m.close()
    _models.clear()


@pytest.fixture
def options(hip_backend):
    yield hip_backend
    hip_backend.set_option(capi.OPT_FUSE_RESIDENT_WGS, -1)
    hip_backend.set_option(capi.OPT_ATTN_SPLIT_MIN_KEYS, -1)


def _run(be, m, n, tokens=None):
    """n greedy vtable steps of a fresh session from token 3 (fed `tokens` instead of its own picks when given)
    -> (picks, logits [n, vocab], launches per step)"""
    s = llama.Session(m, llama.hip_backend_fns(be))
    tok, picks, logits = 3, [], []
    for pos in range(n):
        t, l = s.step(tok, pos)
        assert not be.last_error(), (pos, be.last_error())
        picks.append(t), logits.append(l)
        tok = t if tokens is None else tokens[pos]
    launches = capi.load_hip().zgml_hip_get_runtime_profile(be.ctx, s.handle).contents.backend_dispatch_count // n
    s.close()
    return picks, np.stack(logits), launches


def _fused_against_refused(be, name, kvq, n, exact, own=""):
    m = _model(name, kvq, own)
    picks, logits, launches = _run(be, m, n)
    assert np.isfinite(logits).all()
    be.set_option(capi.OPT_FUSE_RESIDENT_WGS, 0)
    picks_u, logits_u, launches_u = _run(be, m, n, tokens=picks)
    print(f"{name} kvq={kvq} n={n}: launches per step {launches} fused / {launches_u} refused")
    assert launches_u == launches + 2, "the fused launch under test was not built"
    err = (np.abs(logits_u - logits).max(axis=1) / np.abs(logits).max(axis=1)).max()
    print(f"{name} kvq={kvq} n={n}: fused against refused, worst |diff| / range = {err:.3g}")
    if exact:
        assert np.array_equal(logits_u, logits)
    else:
        assert err < 2e-5
    assert picks_u == picks


@fused_switch_on
@pytest.mark.gpu
@pytest.mark.parametrize("name,kvq", [("smollm", 0), ("smollm", 32), ("dh128", 32), ("dh128", 0)])
def test_fused_against_refused_split32(options, name, kvq):
    """80 vtable steps with the split threshold at 32 keys; the same tokens through the plan with the fusion refused. Bit-equal
    logits but for d_head 128 with f32 KV, whose refused plan runs 256-thread workgroups and so another sum: that leg is held to
    2e-5 of the logit range (the bar and the reason of tests/test_hip_qkv_colocate.py). Equal picks, no error word."""
    options.set_option(capi.OPT_ATTN_SPLIT_MIN_KEYS, 32)
    _fused_against_refused(options, name, kvq, 80, exact=not (name == "dh128" and kvq == 0))


@fused_switch_on
@pytest.mark.gpu
def test_fused_against_refused_default_split(options):
    """Positions 0..199 at the default split threshold (SmolLM, f32 KV): up to 13 waves wait behind the sweeping wave, no split is live.
    On a model of its own: a program whose plan was rebuilt (a changed fusion option) after it had seen only 80 keys takes that
    for the bound of its launch schedule and runs in program order, one launch per op, beyond it — no fused launch to test."""
    _fused_against_refused(options, "smollm", 0, 200, exact=True, own="default-split")


@fused_switch_on
@pytest.mark.gpu
def test_ring_under_graph_replay(options):
    """Two calls of the resident loop over positions 0..199 on one session: 400 graph replays, the wait's state is per execution,
    the generations run on. Each call gives the vtable path's tokens and no wait times out."""
    be = options
    s = llama.Session(_model("smollm", 0, own="replay"), llama.hip_backend_fns(be))  # (a program no option change has rebuilt)
    try:
        s.resident_setup(be)
        for call in range(2):
            got = s.resident_decode(3, 0, 200)  # (raises on a time-out: the call returns -1)
            assert not be.last_error(), (call, be.last_error())
            want, _ = s.decode(3, 0, 200)
            assert not be.last_error(), (call, be.last_error())
            assert got.tolist() == want.tolist(), call
    finally:
        s.close()
