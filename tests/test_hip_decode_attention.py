"""The fused decode attention (zgml_amd/csrc/attention_decode.h) on the device, through the case table of
tests/decode_attention_cases.py (pinned on the CPU by tests/test_decode_attention_cases_host.py): every stand-alone instantiation
at its cuts — one launch, the roped q / k and both caches bit-equal to the oracle, the head outputs and their row-store copies
within ATOL = 2e-5 of float64 attention over those buffers, sentinels untouched, nothing non-finite — and the two fused
q / k / v + attention launches (qmatvec.hip qkv_attn_kernel, qkv_attn_kon_kernel), whose attention is compared with float64
attention over the device's own q and caches at the positions the body's geometry gives.
ZGML_HIP_ATTN_DECODE_BLOCK is latched per process: the forced workgroup sizes run in a child pytest each."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from zgml_amd import DeviceOp, capi, llama
from tests import attention_cases as AC
from tests import decode_attention_cases as DC

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = Path(__file__).resolve().parent.parent
BLOCK_ENV = int(os.environ.get("ZGML_HIP_ATTN_DECODE_BLOCK") or 0)


def bits(a):
    return a.view(np.uint32)


def check_case(hip_backend, oracle, name):
    c, want = DC.oracle_run(oracle, name)
    assert hip_backend.supportsProgram(c.prog)
    hip_backend.set_option(capi.OPT_ATTN_SPLIT_MIN_KEYS, c.min_keys)
    try:
        got, text = DC.run_steps(hip_backend, c, executes=lambda st: 2 if st.twice else 1)
        assert not hip_backend.last_error(), hip_backend.last_error()
    finally:
        hip_backend.set_option(capi.OPT_ATTN_SPLIT_MIN_KEYS, -1)
    lines = text.splitlines()
    tagged = [ln for ln in lines if " decode-attention heads " in ln]
    assert len(tagged) == 1 and not [ln for ln in lines if "attention-" in ln] and len(lines) == 1, text
    assert f"heads {c.n_heads}" + (" kvq" if c.form.kvq else "") in tagged[0] and f"ops {len(c.prog.ops)} " in tagged[0], text
    written = c.written()
    worst, worst_at, x_max, v_max = 0.0, "", 0.0, 0.0
    for st in c.steps:
        g, w = got[st.name], want[st.name]
        what = f"{name} {st.name} (seq_kv {st.seq_kv}, column {st.col})"
        for b, label in ((DC.QR, "roped q"), (DC.KR, "roped k"), (DC.KC, "K cache"), (DC.VC, "V cache")):
            diff = np.flatnonzero(bits(g[b]) != bits(w[b]))
            assert diff.size == 0, f"{what}: {label} differs from the oracle's bits at {diff[:8]} ({diff.size} words)"
        ref = DC.float64_heads(c, st, want[st.clean_of] if st.poison else w)
        x, v = DC.live_stats(c, st, want[st.clean_of] if st.poison else w)
        x_max, v_max = max(x_max, x), max(v_max, v)
        for b, idx in written.items():
            out = g[b][idx].reshape(c.n_heads, c.form.d_head)
            assert np.isfinite(out).all(), f"{what}: buffer {b} has {np.count_nonzero(~np.isfinite(out))} non-finite values"
            err = float(np.abs(out - ref).max())
            if err > worst:
                worst, worst_at = err, st.name
            assert err <= DC.ATOL, f"{what}: buffer {b} off by {err:.3g} (head {int(np.abs(out - ref).max(axis=1).argmax())})"
            if st.zero:
                assert np.all(out == 0), what
            keep = np.ones(g[b].size, bool)
            keep[idx] = False
            assert np.all(g[b][keep] == DC.SENTINEL), f"{what}: buffer {b} sentinels overwritten"
    print(f"PARITY {name}: worst |device - float64| = {worst:.3g} at {worst_at} (bar {DC.ATOL:g}, margin {DC.ATOL / max(worst, 1e-30):.1f}x); "
          f"largest |score - max| = {x_max:.2f}, max |V| = {v_max:.2f}")


@pytest.mark.parametrize("name", DC.DEFAULT_CASES)
def test_standalone_case(hip_backend, oracle, name):
    check_case(hip_backend, oracle, name)


if BLOCK_ENV in DC.FORCED:  # (the child of test_forced_block_size: the process has the size latched)
    @pytest.mark.parametrize("name", DC.forced_cases(BLOCK_ENV))
    def test_forced_case(hip_backend, oracle, name):
        check_case(hip_backend, oracle, name)


@pytest.mark.parametrize("block_env", sorted(DC.FORCED))
def test_forced_block_size(block_env):
    """d_head 64 in 256-thread workgroups, d_head 128 in 1024-thread ones: the same checks in a process of their own"""
    ids = [f"{Path(__file__)}::test_forced_case[{n}]" for n in DC.forced_cases(block_env)]
    assert ids
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-s", *ids], capture_output=True, text=True, timeout=300,
                       cwd=ROOT, env=dict(os.environ, ZGML_HIP_ATTN_DECODE_BLOCK=str(block_env)))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert f"{len(ids)} passed" in r.stdout, r.stdout[-2000:]
    print("".join(ln + "\n" for ln in r.stdout.splitlines() if ln.startswith("PARITY")), end="")


# ── the two fused launches (decode_attention_cases.FUSED_MODELS) ───────────────────────────────────────────────────────────

def _download(hip_backend, handle, buf, n):
    out = np.zeros(n, f32)
    io = (capi.ProgramIOC * 1)(capi.ProgramIOC(buf, 0, 0, out.ctypes.data, 4 * n, 0))
    capi.load_hip().zgml_hip_download_outputs(hip_backend.ctx, handle, io, 1)
    assert not hip_backend.last_error(), hip_backend.last_error()
    return out


def _attention_ops(m):
    prog, out = m.program, []
    for i in range(prog.n_ops):
        op = prog.ops[i]
        for kind in ("attention", "attention_kvq"):
            if op.kind == capi.DOP[kind]:
                st = getattr(op.u, kind)
                out.append(DeviceOp(kind, **{n: getattr(st, n) for n, _ in st._fields_ if not n.startswith("_")}))
    return out


@pytest.mark.parametrize("kvq", [0, 32])
@pytest.mark.parametrize("name", sorted(DC.FUSED_MODELS))
def test_fused_launch_attention(hip_backend, name, kvq):
    """The attention inside the q / k / v projection launch, isolated from the mat-vec's summation order: at each position the
    layer's destination against float64 attention over the device's own roped q, caches and mask row."""
    d_model, n_heads, n_kv, d_ff, n_layers, block, n_fused = DC.FUSED_MODELS[name]
    form, S, max_seq, check = DC.fused_plan(name, kvq)
    cfg = llama.preset("smollm-135m", max_seq)
    cfg.d_model, cfg.n_heads, cfg.n_kv_heads, cfg.d_ff, cfg.n_layers, cfg.vocab_size, cfg.kv_quant_block = d_model, n_heads, n_kv, d_ff, n_layers, 256, kvq
    m = llama.Model(cfg, llama.Q4_0, threads=8)
    fns = llama.hip_backend_fns(hip_backend)
    hip_backend.set_option(capi.OPT_ATTN_SPLIT_MIN_KEYS, DC.MIN_KEYS)
    s = None
    try:
        hip_backend.set_option(capi.OPT_FUSE_RESIDENT_WGS, 0)  # the same program with the fusion refused: one launch more per fused layer
        try:
            s_u = llama.Session(m, fns)
            plain = hip_backend.planText(s_u.handle).splitlines()
            s_u.close()
        finally:
            hip_backend.set_option(capi.OPT_FUSE_RESIDENT_WGS, -1)
        s = llama.Session(m, fns)
        text = hip_backend.planText(s.handle)
        lines = text.splitlines()
        n_adec = lambda ls: len([ln for ln in ls if " decode-attention heads " in ln])  # noqa: E731
        assert n_adec(plain) == n_layers and n_adec(lines) == n_layers - n_fused and len(lines) == len(plain) - n_fused, text
        worst, worst_at, tok = 0.0, None, 3
        sizes = m.program.buffer_sizes
        for pos in range(check[-1]):
            tok, _ = s.step(tok, pos)
            assert not hip_backend.last_error(), hip_backend.last_error()
            if pos + 1 not in check:
                continue
            ops = _attention_ops(m)
            assert len(ops) == n_layers * n_heads and all(o.f["seq_kv"] == pos + 1 and o.f["seq_q"] == 1 for o in ops)
            bufs = {}
            for o in ops:
                for b in (o.f["q"], o.f["k"], o.f["v"], o.f["mask"], o.f["dst"]):
                    if b not in bufs:
                        bufs[b] = _download(hip_backend, s.handle, b, int(sizes[b]))
            for o in ops:
                with np.errstate(invalid="ignore", over="ignore"):
                    want = AC.float64_attention(o, bufs, pos + 1)[0]
                out = AC.gather_out(o, bufs[o.f["dst"]])[0]
                assert np.isfinite(out).all(), (name, kvq, pos)
                err = float(np.abs(out - want).max())
                if err > worst:
                    worst, worst_at = err, pos + 1
                assert err <= DC.ATOL, f"{name} kvq {kvq} seq_kv {pos + 1}: head at q_off {o.f['q_off']} off by {err:.3g}"
    finally:
        hip_backend.set_option(capi.OPT_ATTN_SPLIT_MIN_KEYS, -1)
        if s:
            s.close()
        m.close()
    print(f"PARITY fused {name} {form.tag} S {S}: worst |device - float64| = {worst:.3g} at seq_kv {worst_at} over {check} "
          f"(bar {DC.ATOL:g}, margin {DC.ATOL / max(worst, 1e-30):.1f}x)")
