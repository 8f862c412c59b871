"""The block map of the fused q / k / v + decode attention launch (zgml_amd/csrc/qkv_colocate.h, qmatvec.hip qkv_attn_kernel): a kv
group's projection column groups and split 0 of its heads carry one label `block id % 8`, so that the head-local hand-off stays
inside one XCD. Which block plays which role may change speed and nothing else: the granules carry their generation, any
placement gives the same bits.

Models of one and two layers at SmolLM-135M's layer dimensions (d 576, 9 x 64, 3 kv heads) with f32 and int8 KV, and at
d_head 128 with n-on-lanes weights (d 768, 6 x 128, 6 kv heads; int8 KV, and f32 KV: REFUSED_IS_ANOTHER_SUM); vocabulary 2048. max_seq is 2048, so the default plan has 16
splits per head and the map is ON (9, 3, 64, 16 and 6, 6, 128, 16 in tests/test_qkv_colocate_host.py); with a resident-workgroup
capacity of projection workgroups + one per head the launch has ONE split and the map is the identity (9, 3, 64, 1 and
6, 6, 128, 1 there); one workgroup less and the fusion is refused. The three plans run the same arithmetic in the same order."""
import os

import numpy as np
import pytest

from zgml_amd import capi, llama

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(os.environ.get("ZGML_HIP_FUSE_QKV_ATTN") == "0",
                                                  reason="the diagnostic switch under test turns the fused launch off")]

VARIANTS = [("smollm", 1, 0), ("smollm", 2, 0), ("smollm", 1, 32), ("smollm", 2, 32), ("dh128", 2, 32), ("dh128", 2, 0)]
N = 80
# d_head 128 with f32 KV: the STAND-ALONE decode attention of the refused plan runs 256-thread workgroups there (kernels_generic.hip
# launch_attention_decode_batch), the fused launch 1024-thread ones — the waves cut the keys differently, so that one plan is not the
# same arithmetic as the other two, whatever the placement. Its refused leg is held to tests/test_hip_fused_qkv.py's bound for the
# same pair of plans (2e-5 of the logit range; measured here: 3.7e-7 absolute on logits of 0.25); every other comparison of every
# variant, the fused legs of this one included, is bit for bit.
REFUSED_IS_ANOTHER_SUM = {("dh128", 2, 0)}


def _cfg(name, layers, kvq):
    cfg = llama.preset("smollm-135m", 2048)
    if name == "dh128":  # -> qkv_attn_kernel<..., 32, ...>; 18 x 8 = 144 projection workgroups
        cfg.d_model, cfg.n_heads, cfg.n_kv_heads, cfg.d_ff = 768, 6, 6, 1536
    cfg.n_layers, cfg.vocab_size, cfg.kv_quant_block = layers, 2048, kvq
    return cfg


_models = {}


def _model(variant):
    if variant not in _models:
        _models[variant] = llama.Model(_cfg(*variant), llama.Q4_0, threads=8)
    return _models[variant]


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


def _dispatches(be, s):
    return capi.load_hip().zgml_hip_get_runtime_profile(be.ctx, s.handle).contents.backend_dispatch_count


def _run(be, m, tokens=None):
    """N greedy vtable steps of a fresh session from token 3 (fed `tokens` instead of its own picks when given)
    -> (picks, logits [N, vocab], launches per step); a hand-off that times out is an error of the step"""
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


@pytest.mark.parametrize("variant", VARIANTS)
def test_placement_independence(options, variant):
    """Tokens and every logit of 80 positions: the default plan (map on), one split per head (identity map) and the fusion refused
    are bit-equal (d_head 128 with f32 KV: the refused plan's other sum, REFUSED_IS_ANOTHER_SUM), and no hand-off wait times out."""
    be, m = options, _model(variant)
    cfg = m.cfg
    n_mv = (cfg.n_heads + 2 * cfg.n_kv_heads) * cfg.d_head // 16
    picks, logits, launches = _run(be, m)
    assert np.isfinite(logits).all()
    be.set_option(capi.OPT_FUSE_RESIDENT_WGS, n_mv + cfg.n_heads)
    picks_1, logits_1, launches_1 = _run(be, m, tokens=picks)
    be.set_option(capi.OPT_FUSE_RESIDENT_WGS, n_mv + cfg.n_heads - 1)
    picks_u, logits_u, launches_u = _run(be, m, tokens=picks)
    print(f"{variant}: launches {launches} / {launches_1} / {launches_u}; worst |diff| one split {np.abs(logits_1 - logits).max():.3g}, "
          f"refused {np.abs(logits_u - logits).max():.3g}")
    assert launches_1 == launches and launches_u == launches + cfg.n_layers, "the fused launch under test was not built"
    assert picks_1 == picks and picks_u == picks
    assert np.array_equal(logits_1, logits)
    if variant in REFUSED_IS_ANOTHER_SUM:
        assert (np.abs(logits_u - logits).max(axis=1) / np.abs(logits).max(axis=1)).max() < 2e-5
    else:
        assert np.array_equal(logits_u, logits)


@pytest.mark.parametrize("variant", VARIANTS)
def test_replay_and_live_splits(options, variant):
    """200 positions with the split threshold at 32 keys: up to six live splits per head, of which split 0 sits with its producers
    and the others do not. Two executions of the resident loop over the same positions (400 graph replays: the generations run
    on) give the vtable path's tokens, and no wait times out (the call raises on a time-out)."""
    be, m = options, _model(variant)
    be.set_option(capi.OPT_ATTN_SPLIT_MIN_KEYS, 32)
    s = llama.Session(m, llama.hip_backend_fns(be))
    try:
        want, _ = s.decode(3, 0, 200)
        assert not be.last_error(), be.last_error()
        s.resident_setup(be)
        for call in range(2):
            got = s.resident_decode(3, 0, 200)
            assert not be.last_error(), (call, be.last_error())
            assert got.tolist() == want.tolist(), call
    finally:
        s.close()
