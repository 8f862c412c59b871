"""Legality of the launch planner's fusions (zgml_amd/csrc/plan.hip). For each pass a positive control — a minimal program
the pass fuses, checked on the plan text — and near misses: the same program with ONE condition broken (an operand that meets
a member's output at a shifted index, a store into the anchor's input, a second reader, misaligned offsets, a barrier). The
plan text must show the ops apart, and every buffer must match the oracle. The elementwise and row-chain race cases are sized
so that a wrong fusion shows: a grid far above what the device keeps resident and a forward shift of about half the grid (the
reader finishes before the writer's workgroup starts). The mat-vec, store-fold and decode-attention cases run grids the device
holds at once, where a race seldom shows in the numbers: there the plan-text assertion is what guards them.
Positive controls of the passes over the launch list (arm_prenorm, arm_pair, fuse_qkv_attention) live with their kernels'
tests (tests/test_hip_qmatvec.py, tests/test_hip_fused_qkv.py).

Also pinned: the plan shape of the product programs (tiny / SmolLM-135M decode, a 32-token prefill chunk), so that a legality
check that refuses too much fails here rather than as a slower benchmark."""
import ctypes as C
import re

import numpy as np
import pytest

from zgml_amd import DeviceOp, DeviceProgram, ProgramIO, capi, llama
from tests.plan_cases import decode_group, group_uploads
from tests.test_hip_qmatvec import _q4_weight

pytestmark = pytest.mark.gpu
f32 = np.float32


def launches(text):
    """plan text -> [(kind, n_ops, lo, hi, rest of the line)]"""
    out = []
    for line in text.splitlines():
        m = re.match(r"\d+: kind (\d+) ops (\d+) \[(\d+)\.\.(\d+)\](.*)", line)
        assert m, line
        out.append((int(m[1]), int(m[2]), int(m[3]), int(m[4]), m[5]))
    return out


def run_both(be, oracle, prog, barriers=()):
    """compile on both backends, execute once, compare EVERY buffer; returns the HIP plan text"""
    ref = oracle.OracleBackend()
    hr = ref.compileProgram(prog)
    be.set_option(capi.OPT_SKIP_DEAD_UPLOADS, 0)  # every buffer stays readable, also one a near miss no longer references
    try:
        h = be.compileProgram(prog)
    finally:
        be.set_option(capi.OPT_SKIP_DEAD_UPLOADS, 1)
    assert h, be.last_error()
    try:
        if barriers:
            arr = (C.c_uint64 * len(barriers))(*barriers)
            assert capi.load_hip().zgml_hip_program_set_barriers(be.ctx, h, arr, len(barriers)) == 0
        text = be.planText(h)
        outs = [ProgramIO(b, np.zeros(int(s), f32)) for b, s in enumerate(prog.buffer_sizes)]
        be.executeProgram(h, [], outs)
        ref.executeProgram(hr, [], [])
        assert not be.last_error(), be.last_error()
        for b, io in enumerate(outs):
            want = ref.buffer(hr, b)
            scale = max(1.0, float(np.abs(want).max()))
            np.testing.assert_allclose(io.host, want, rtol=0, atol=1e-4 * scale, err_msg=f"buffer {b}\n{text}")
    finally:
        be.freeProgram(h)
        ref.freeProgram(hr)
    return text


def fused(text, lo, hi, kind=None):
    return any(L[2] == lo and L[3] == hi and L[1] == hi - lo + 1 and (kind is None or L[0] == kind) for L in launches(text))


def values(rng, n, lo=-1.0, hi=1.0):
    return rng.uniform(lo, hi, n).astype(f32)


# ── elementwise chains ─────────────────────────────────────────────────────────────────────────────────────────────────

N_RACE = 1 << 22  # 16 Ki workgroups of 256 threads


@pytest.mark.parametrize("case", ["control", "shifted_operand", "shifted_store", "barrier"])
def test_elementwise_chain(hip_backend, oracle, case):
    """t = x + y; z = t * w. Near misses: w = t[s:] (thread i reads t[i + s], another workgroup's store in the same launch),
    z stored into t[s:], and a barrier between the two ops."""
    rng = np.random.default_rng(1)
    n, s = N_RACE, N_RACE // 2
    X, Y, T, W, Z = range(5)
    sizes = [n, n, n + s, n, n + s]
    op0 = DeviceOp.elementwise("add", T, X, Y, n)
    op1 = {"control": DeviceOp.elementwise("mul", Z, T, W, n), "barrier": DeviceOp.elementwise("mul", Z, T, W, n),
           "shifted_operand": DeviceOp.elementwise("mul", Z, T, T, n, src1_offset=s),
           "shifted_store": DeviceOp.elementwise("mul", T, T, W, n, dst_offset=s)}[case]
    ups = [ProgramIO(X, values(rng, n)), ProgramIO(Y, values(rng, n)), ProgramIO(T, values(rng, n + s, 5, 6)), ProgramIO(W, values(rng, n)),
           ProgramIO(Z, values(rng, n + s))]
    text = run_both(hip_backend, oracle, DeviceProgram([op0, op1], sizes, ups), barriers=(1,) if case == "barrier" else ())
    assert fused(text, 0, 1, 11) == (case == "control"), text


# ── [add ->] rmsnorm [-> mul] row chains ───────────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("case", ["control", "gain_rows_ahead", "gain_is_sum", "store_rows_ahead"])
def test_row_chain(hip_backend, oracle, case):
    """h = x + y; n = rmsnorm(h); o = n * g over 8192 rows. Near misses: g = h shifted by half the rows (a row reads another
    row's sum, stored by another workgroup of the same launch), g = h itself (the launch reads its inputs up front, before the
    add's store), o stored half the rows ahead into h."""
    rng = np.random.default_rng(2)
    rows, cols = 8192, 256
    n, s = rows * cols, rows // 2 * cols
    X, Y, H, NRM, G, O = range(6)
    sizes = [n, n, n + s, n, n, n + s]
    mul = {"control": DeviceOp.elementwise("mul", O, NRM, G, n), "gain_rows_ahead": DeviceOp.elementwise("mul", O, NRM, H, n, src1_offset=s),
           "gain_is_sum": DeviceOp.elementwise("mul", O, NRM, H, n), "store_rows_ahead": DeviceOp.elementwise("mul", H, NRM, G, n, dst_offset=s)}[case]
    ops = [DeviceOp.elementwise("add", H, X, Y, n), DeviceOp.rmsnorm(NRM, H, rows, cols, 1e-5), mul]
    ups = [ProgramIO(X, values(rng, n)), ProgramIO(Y, values(rng, n)), ProgramIO(H, values(rng, n + s, 3, 4)), ProgramIO(NRM, values(rng, n)),
           ProgramIO(G, values(rng, n)), ProgramIO(O, values(rng, n + s))]
    text = run_both(hip_backend, oracle, DeviceProgram(ops, sizes, ups))
    assert fused(text, 0, 2, 5) == (case == "control"), text


# ── mat-vec epilogues ──────────────────────────────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("case", ["control", "into_input", "shifted_operand", "misaligned_input"])
def test_matvec_epilogue(hip_backend, oracle, case):
    """y = W x; z = y + r. Near misses: z stored into x (x = W x + r: every workgroup reads all of x while the owners of the
    columns store into it), r = y shifted by half the columns, an input offset that is not a multiple of 4 (no fusion at all)."""
    rng = np.random.default_rng(3)
    K = N = 2048
    Xb, Yb, R, Z = range(4)
    sizes = [K + 4, N + N // 2, N, N]
    qm = DeviceOp.qmatmul(Yb, Xb, 0, 1, N, K, input_offset=2 if case == "misaligned_input" else 0)
    epi = {"control": DeviceOp.elementwise("add", Z, Yb, R, N), "misaligned_input": DeviceOp.elementwise("add", Z, Yb, R, N),
           "into_input": DeviceOp.elementwise("add", Xb, Yb, R, N), "shifted_operand": DeviceOp.elementwise("add", Z, Yb, Yb, N, src1_offset=N // 2)}[case]
    ups = [ProgramIO(Xb, values(rng, K + 4)), ProgramIO(Yb, values(rng, N + N // 2, 2, 3)), ProgramIO(R, values(rng, N)), ProgramIO(Z, values(rng, N))]
    text = run_both(hip_backend, oracle, DeviceProgram([qm, epi], sizes, ups, qweights=[_q4_weight(rng, K, N)]))
    assert fused(text, 0, 1, 2) == (case == "control"), text


# ── mat-vec prologues ──────────────────────────────────────────────────────────────────────────────────────────────────

def _pro(text):
    return [L[4] for L in launches(text) if " qmv " in L[4]]


@pytest.mark.parametrize("case", ["control_mul", "control_rmsnorm", "gain_over_norm", "in_place_mul", "second_reader", "input_overwritten",
                                  "misaligned", "barrier"])
def test_matvec_prologue(hip_backend, oracle, case):
    """[n = rmsnorm(h);] xg = n * g; y = W xg. Near misses: the gain reads the norm's output 4 elements on (workgroup 0 stores
    the norm while every workgroup reads the gain), xg = xg * g in place, a second reader of the norm's output, the mul's input
    overwritten between two consumers, an offset that is not a multiple of 4, a barrier between the mul and the mat-vec."""
    rng = np.random.default_rng(4)
    K, N = 1024, 512
    Hb, NRM, G, XG, Y, Y2, Z = range(7)
    sizes = [K, K + 4, K, K, N, N, K]
    norm = DeviceOp.rmsnorm(NRM, Hb, 1, K, 1e-5)
    mul = DeviceOp.elementwise("mul", XG, NRM, G, K)
    qm = DeviceOp.qmatmul(Y, XG, 0, 1, N, K)
    barriers = ()
    if case == "control_mul":
        ops, want = [mul, qm], "pro mul"
    elif case == "control_rmsnorm":
        ops, want = [norm, mul, qm], "pro rmsnorm"
    elif case == "gain_over_norm":  # the rmsnorm form is refused; the plain mul form (its store meets no input) remains
        ops, want = [norm, DeviceOp.elementwise("mul", XG, NRM, NRM, K, src1_offset=4), qm], "pro mul"
    elif case == "in_place_mul":
        ops, want = [DeviceOp.elementwise("mul", XG, XG, G, K), qm], None
    elif case == "second_reader":
        ops, want = [norm, mul, qm, DeviceOp.elementwise("add", Z, NRM, G, K)], "pro mul"
    elif case == "input_overwritten":
        ops, want = [mul, qm, DeviceOp.elementwise("add", G, G, Hb, K), DeviceOp.qmatmul(Y2, XG, 1, 1, N, K)], None
    elif case == "misaligned":
        ops, want = [DeviceOp.elementwise("mul", XG, NRM, G, K - 4, dst_offset=2, src0_offset=2), DeviceOp.qmatmul(Y, XG, 0, 1, N, K - 4, input_offset=2)], None
    else:
        ops, want, barriers = [mul, qm], None, (1,)
    ups = [ProgramIO(Hb, values(rng, K)), ProgramIO(NRM, values(rng, K + 4)), ProgramIO(G, values(rng, K, 0.5, 1.5)), ProgramIO(XG, values(rng, K)),
           ProgramIO(Y, values(rng, N)), ProgramIO(Y2, values(rng, N)), ProgramIO(Z, values(rng, K))]
    qk = K - 4 if case == "misaligned" else K
    prog = DeviceProgram(ops, sizes, ups, qweights=[_q4_weight(rng, qk, N), _q4_weight(rng, qk, N)])
    text = run_both(hip_backend, oracle, prog, barriers)
    pros = _pro(text)
    if want:
        assert any(want in p for p in pros), text
        if want == "pro mul":
            assert not any("pro rmsnorm" in p or "pro prenorm" in p for p in pros), text
    else:
        assert not any("pro mul" in p or "pro rmsnorm" in p or "pro prenorm" in p for p in pros), text


# ── decode attention and the store folds ───────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("case", ["control", "k_source_overwritten", "row_store_other_offset", "row_store_over_cache", "no_mask"])
def test_decode_attention_group(hip_backend, oracle, case):
    """rope q / k, K / V stores, per-head attention and row store of one kv group: one decode-attention launch of all 3 + 3h
    ops. Near misses: the rotated k (the K store's source) overwritten between the store and the attentions, a row store that
    reads its head's output 4 elements on (no fold: that row store stays out of the launch), the last head's row store into
    a column of the K cache that the other head's attention reads in the same launch."""
    rng = np.random.default_rng(6)
    nh, pos = 2, 3
    ops, sizes = decode_group(n_heads=nh, pos=pos, has_mask=case != "no_mask")
    KR, KC, AO = 3, 4, 7
    n_group = len(ops)
    if case == "k_source_overwritten":
        ops.insert(nh + 2, DeviceOp.elementwise("neg", KR, KR, KR, 64))
    elif case == "row_store_other_offset":
        ops[-1] = ops[-1].with_(src_offset=ops[-1].src_offset + 4)
    elif case == "row_store_over_cache":
        ops[-1] = ops[-1].with_(dst=KC, dst_base_offset=64, dst_offset=64)  # column 1, which head 0 reads
    prog = DeviceProgram(ops, sizes, group_uploads(rng, sizes, pos))
    text = run_both(hip_backend, oracle, prog)
    adec = [L for L in launches(text) if "decode-attention" in L[4]]
    if case in ("control", "no_mask"):
        assert len(adec) == 1 and adec[0][1] == n_group, text
    elif case == "row_store_other_offset":  # the group fuses without the row store that reads elsewhere
        assert len(adec) == 1 and adec[0][1] == n_group - 1, text
    else:
        assert not adec, text


@pytest.mark.parametrize("anchor", ["rope", "attention"])
@pytest.mark.parametrize("case", ["control", "slice_over_source"])
def test_store_fold(hip_backend, oracle, anchor, case):
    """rope (seq 4) -> slice_assign of its rows, attention (seq_q 4) -> slice_assign of its head output: one launch each.
    Near miss: the slice lands on the anchor's own source at another index (the anchor stores both copies per element while
    other threads of the launch still read that source)."""
    rng = np.random.default_rng(7)
    dh, seq = 16, 4
    if anchor == "rope":
        # 0 src, 1 cos|sin, 2 rotated, 3 slice destination
        op = DeviceOp.rope(2, 0, 1, dh // 2, seq, 0, 0, 0, 1, dh, dh)
        dst, dst_off = (0, 8) if case == "slice_over_source" else (3, 0)
        sl = DeviceOp.slice_assign(dst, 2, dh, seq, dst_off, dst_off, 1, dh, 0, 1, dh, 0)
        sizes = [dh * seq + 8, dh * seq, dh * seq, dh * seq]
    else:
        # 0 q, 1 k, 2 v, 3 mask, 4 out, 5 slice destination
        op = DeviceOp.attention(4, 0, 1, 2, 3, False, dh, seq, 6, 0.25, 0, 0, 0, 0, 0, 1, dh, 1, dh, 1, dh, 1, 1, 1, dh)
        dst, dst_off = (1, 8) if case == "slice_over_source" else (5, 0)
        sl = DeviceOp.slice_assign(dst, 4, dh, seq, dst_off, dst_off, 1, dh, 0, 1, dh, 0)
        sizes = [dh * seq, dh * 6 + 8, dh * 6, 1, dh * seq, dh * seq]
    ups = [ProgramIO(b, values(rng, sz)) for b, sz in enumerate(sizes)]
    text = run_both(hip_backend, oracle, DeviceProgram([op, sl], sizes, ups))
    assert fused(text, 0, 1) == (case == "control"), text


# ── the refresh contract meets legality: a static refresh that turns a fused chain into a near miss ─────────────────────

def test_static_refresh_rechecks_legality(hip_backend, oracle):
    rng = np.random.default_rng(5)
    n, s = N_RACE, N_RACE // 2
    X, Y, T, W, Z = range(5)
    sizes = [n, n, n + s, n, n + s]
    ops = [DeviceOp.elementwise("add", T, X, Y, n), DeviceOp.elementwise("mul", Z, T, W, n)]
    near = [ops[0], DeviceOp.elementwise("mul", Z, T, T, n, src1_offset=s)]
    ups = [ProgramIO(X, values(rng, n)), ProgramIO(Y, values(rng, n)), ProgramIO(T, values(rng, n + s, 5, 6)), ProgramIO(W, values(rng, n)),
           ProgramIO(Z, values(rng, n + s))]
    prog = DeviceProgram(ops, sizes, ups)
    ref = oracle.OracleBackend()
    hr = ref.compileProgram(prog)
    hip_backend.set_option(capi.OPT_SKIP_DEAD_UPLOADS, 0)
    try:
        h = hip_backend.compileProgram(prog)
    finally:
        hip_backend.set_option(capi.OPT_SKIP_DEAD_UPLOADS, 1)
    try:
        assert fused(hip_backend.planText(h), 0, 1, 11)
        outs = [ProgramIO(b, np.zeros(sz, f32)) for b, sz in enumerate(sizes)]
        hip_backend.executeProgram(h, [], outs)
        ref.executeProgram(hr, [], [])
        hip_backend.refreshProgram(h, near)
        ref.refreshProgram(hr, near)
        text = hip_backend.planText(h)
        assert not fused(text, 0, 1), text
        hip_backend.executeProgram(h, [], outs)
        ref.executeProgram(hr, [], [])
        assert not hip_backend.last_error(), hip_backend.last_error()
        for b, io in enumerate(outs):
            np.testing.assert_allclose(io.host, ref.buffer(hr, b), rtol=0, atol=1e-4 * 40, err_msg=f"buffer {b}")
    finally:
        hip_backend.freeProgram(h)
        ref.freeProgram(hr)


# ── plan-shape pins of the product programs ────────────────────────────────────────────────────────────────────────────

def plan_shape(text):
    """launch count, and how many launches carry each fused form"""
    ls = launches(text)
    forms = {}
    for L in ls:
        for tag in ("pro mul", "pro rmsnorm", "pro prenorm", "prepares-next-norm", " pair", "+decode-attention", " decode-attention"):
            if tag in L[4]:
                forms[tag.strip()] = forms.get(tag.strip(), 0) + 1
        if L[1] > 1 and " qmv " not in L[4] and "decode-attention" not in L[4]:
            forms[f"kind{L[0]}x"] = forms.get(f"kind{L[0]}x", 0) + 1  # a multi-op launch of another kind (chains, batches)
    return len(ls), forms


# (preset, token_len) -> (launches, fused forms) as the planner builds them (max_seq 64)
PINS = {("tiny", 1): (12, {"pro rmsnorm": 1, "decode-attention": 2, "prepares-next-norm": 3, "pro prenorm": 3, "pair": 2, "kind5x": 1}),
        ("smollm-135m", 1): (122, {"kind2x": 30, "prepares-next-norm": 59, "pro prenorm": 30, "pair": 30, "kind5x": 1}),
        ("tiny", 32): (20, {"kind5x": 5, "kind2x": 4, "kind8x": 2, "kind10x": 2, "kind11x": 2})}


@pytest.mark.parametrize("name,token_len", [("tiny", 1), ("smollm-135m", 1), ("tiny", 32)])
def test_product_plan_shapes(hip_backend, name, token_len):
    cfg = llama.preset(name, 64)
    m = llama.Model(cfg, llama.Q4_0, threads=8, token_len=token_len)
    s = llama.Session(m, llama.hip_backend_fns(hip_backend))
    try:
        if token_len == 1:
            s.step(3, 0)
        else:
            s.prefill([(7 * i + 3) % cfg.vocab_size for i in range(token_len)], 0)
        assert not hip_backend.last_error(), hip_backend.last_error()
        got = plan_shape(hip_backend.planText(s.handle))
        assert got == PINS[(name, token_len)], got
    finally:
        s.close(), m.close()
