"""Who owns the resident state, on the MI355X (zgml_amd/csrc/dev_block.h, runtime_internal.h: GraphSlot; the rules themselves are
held on the CPU by tests/test_dev_block_host.py):

1. A resident set-up that fails publishes nothing: the program has no set-up afterwards, whatever it had before, and the next
   good set-up works. Host-side refusals throughout: nothing is launched.
2. The tables that lie next to the produced tokens grow with a longer call; the graphs that baked them are captured again and
   nothing else moves: every call of a 4 / 40 / 4 sequence of the sampled loop (picks, log-probabilities, alternatives), with the
   greedy loop in between, equals the same call on a fresh session to the bit, and a step is as many launches as before.
3. The same for the verify loop (greedy and sampled) on a token_len = 3 plan; the batched verify loop on ANOTHER program keeps its
   graph over all of it, and captures again when its own table grows."""
import ctypes as C

import numpy as np
import pytest

from zgml_amd import DeviceOp, DeviceProgram, ProgramIO, capi, llama
from tests.test_hip_sample import FIRST, PARAMS, PROMPT_LEN, session_behind_prompt, tiny
from tests.test_hip_spec_decode import FIRST_AT_0, spec_session
from tests.test_sample_host import c_sample

pytestmark = pytest.mark.gpu

f32 = np.float32
S = capi.SamplingC.of
SP = dict(seed=1234, stream=0, **PARAMS["k40_p95"])
SHORT, LONG = 4, 40


def _profile(be, handle):
    p = be.getRuntimeProfile(handle)
    return int(p.backend_dispatch_count), int(p.call_count)


def _counted(be, handle, call):
    """-> (what `call` returned, launches per step of it, steps)"""
    d0, c0 = _profile(be, handle)
    got = call()
    d1, c1 = _profile(be, handle)
    assert not be.last_error(), be.last_error()
    assert c1 > c0 and (d1 - d0) % (c1 - c0) == 0
    return got, (d1 - d0) // (c1 - c0), c1 - c0


def _same(a, b):
    """bit for bit, through tuples / lists / dicts of arrays and numbers"""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


# ── 1. a failed set-up publishes nothing ───────────────────────────────────────────────────────────────────────────────

def _setup(be, h, n, n_rope, rope_buf=0):
    embed, tab = np.zeros(n, f32), np.zeros(1, f32)
    ropes = (C.c_uint16 * 1)(rope_buf)
    d = capi.ResidentLlamaC()
    d.token_embed, d.cos_table, d.sin_table = embed.ctypes.data, tab.ctypes.data, tab.ctypes.data
    d.vocab, d.d_model, d.max_seq, d.d_head = n, 1, 1, 1
    d.buf_token_input, d.buf_attn_mask, d.buf_logits = 1, 1, 0
    d.buf_rope, d.n_rope = C.cast(ropes, C.POINTER(C.c_uint16)), n_rope
    return capi.load_hip().zgml_hip_resident_setup(be.ctx, h, C.byref(d))


def test_a_failed_setup_publishes_nothing(hip_backend):
    be, hip = hip_backend, capi.load_hip()
    vec = np.linspace(-2.0, 3.0, 8).astype(f32)

    def no_setup(h):
        assert hip.zgml_hip_program_set_constraint(be.ctx, h, 0, None, 0) == -1
        assert "no resident set-up" in be.last_error()
        hip.zgml_hip_clear_error(be.ctx)

    def bad_setup(h):
        assert _setup(be, h, vec.size, n_rope=1, rope_buf=2) == -1  # (the program has buffers 0 and 1)
        assert "bad rope buffer" in be.last_error()
        hip.zgml_hip_clear_error(be.ctx)

    # on vector_program's two-buffer program (vocab 8, d_model 1, max_seq 1) before it has a set-up
    h = be.compileProgram(DeviceProgram(ops=[DeviceOp.elementwise("abs", 1, 0, 0, 1)], buffer_sizes=[vec.size, 1], initial_uploads=[ProgramIO(0, vec)]))
    before = _profile(be, h)
    no_setup(h)
    bad_setup(h)
    no_setup(h)  # (the parent of this change answered 0 here: a half-built set-up was published)
    # behind a good one: the good one goes first, as it always did, and nothing takes its place
    assert _setup(be, h, vec.size, n_rope=0) == 0, be.last_error()
    assert hip.zgml_hip_program_set_constraint(be.ctx, h, 0, None, 0) == 0
    bad_setup(h)
    no_setup(h)
    assert _profile(be, h) == before  # host-side refusals: nothing was launched
    # ... and a good set-up after that works
    assert _setup(be, h, vec.size, n_rope=0) == 0, be.last_error()
    assert hip.zgml_hip_program_set_constraint(be.ctx, h, 0, None, 0) == 0
    sp = S(**SP)
    for pos in range(4):
        tok, _ = be.sample(h, 0, 0, vec.size, sp, pos)
        assert tok == c_sample(vec, sp, pos)
    assert not be.last_error(), be.last_error()
    hip.zgml_hip_free_program(be.ctx, h)


# ── 2. grown tables re-capture and nothing else moves: the sampled loop ────────────────────────────────────────────────

KINDS = {"pick": dict(), "logprobs": dict(logprobs=True), "top": dict(logprobs=True, top_logprobs=5)}
_fresh = {}


def _resident(be):
    s, m = session_behind_prompt(be, tiny(), PROMPT_LEN)
    s.resident_setup(be)
    return s, m


def _fresh_sampled(be, kind, n):
    """the call on a session that has run nothing else (computed once per kind and length, left unchanged)"""
    if (kind, n) not in _fresh:
        s, m = _resident(be)
        _fresh[kind, n] = s.resident_decode(FIRST, PROMPT_LEN, n) if kind == "greedy" else s.resident_decode_sampled(FIRST, PROMPT_LEN, n, S(**SP), **KINDS[kind])
        s.close(), m.close()
    return _fresh[kind, n]


def test_grown_tables_recapture_and_nothing_else_moves(hip_backend):
    be = hip_backend
    s, m = _resident(be)
    per_step = {}
    # every kind at 4 steps, then at 40 — each kind's first long call grows a table of its own (the tokens; the values; the
    # pairs) under the graphs of all the others —, then at 4 again; the greedy loop between any two
    for n in (SHORT, LONG, SHORT):
        for kind in KINDS:
            got, launches, steps = _counted(be, s.handle, lambda: s.resident_decode_sampled(FIRST, PROMPT_LEN, n, S(**SP), **KINDS[kind]))
            assert _same(got, _fresh_sampled(be, kind, n)), (kind, n)
            assert got[1] == n and steps == n
            assert per_step.setdefault(kind, launches) == launches, (kind, n)
            greedy, launches, steps = _counted(be, s.handle, lambda: s.resident_decode(FIRST, PROMPT_LEN, SHORT))
            assert _same(greedy, _fresh_sampled(be, "greedy", SHORT)), (kind, n)
            assert steps == SHORT and per_step.setdefault("greedy", launches) == launches, (kind, n)
    # (the values add [partial] and [finish] to the pick's train; the pairs take [finish + top] in the place of [finish])
    assert per_step["logprobs"] == per_step["pick"] + 2 and per_step["top"] == per_step["logprobs"]
    lp = _fresh_sampled(be, "logprobs", LONG)[2]
    assert lp.dtype == f32 and lp.shape == (LONG,) and np.all(np.isfinite(lp)) and np.all(lp <= 0)
    alt_tok, alt_val = _fresh_sampled(be, "top", LONG)[3]
    assert alt_tok.shape == (LONG, 5) and alt_val.shape == (LONG, 5) and np.all(alt_tok >= 0)
    s.close(), m.close()


# ── 3. the same for the verify loop; the batched verify loop's graph is its own ────────────────────────────────────────

T, B, TS = 3, 2, 2
_fresh_spec = {}


def _batch_session(be):
    bm = llama.BatchModel(tiny(), B, llama.Q4_0, tokens_per_seq=TS)
    sb = llama.BatchSession(bm, llama.hip_backend_fns(be), B)
    sb.resident_setup(be)
    return sb, bm


def _spec_call(s, form, n):
    if form == "greedy":
        return s.resident_decode_speculative(FIRST_AT_0, 0, n)
    if form == "sampled":
        return s.resident_decode_speculative_sampled(FIRST_AT_0, 0, n, S(**SP))
    return s.resident_decode_batch_speculative([FIRST_AT_0, FIRST], [0, 0], [n, n])


def _fresh_spec_call(be, form, n):
    if (form, n) not in _fresh_spec:
        s, m = _batch_session(be) if form == "batch" else spec_session(be, tiny(), T)
        _fresh_spec[form, n] = _spec_call(s, form, n)
        s.close(), m.close()
    return _fresh_spec[form, n]


def test_the_verify_loops_grow_alike_and_the_batched_graph_is_its_own(hip_backend):
    be = hip_backend
    s, m = spec_session(be, tiny(), T)
    sb, bm = _batch_session(be)
    per_step = {}

    def check(x, form, n):
        got, launches, steps = _counted(be, x.handle, lambda: _spec_call(x, form, n))
        assert _same(got, _fresh_spec_call(be, form, n)), (form, n)
        assert per_step.setdefault(form, launches) == launches, (form, n)
        return steps

    steps_before = check(sb, "batch", SHORT)
    for n in (SHORT, LONG, SHORT):  # (the long call grows the token table under both forms' graphs)
        for form in ("greedy", "sampled"):
            check(s, form, n)
    assert check(sb, "batch", SHORT) == steps_before  # its graph outlived the growth on the other program
    check(sb, "batch", LONG)  # ... and goes with its own table
    assert check(sb, "batch", SHORT) == steps_before
    toks = _fresh_spec_call(be, "greedy", LONG)[0]
    assert toks.shape == (LONG,) and np.all(toks >= 0)
    assert _fresh_spec_call(be, "sampled", LONG)[1] == LONG
    btoks = _fresh_spec_call(be, "batch", LONG)[0]
    assert btoks.shape == (B, LONG) and np.all(btoks >= 0)
    s.close(), m.close()
    sb.close(), bm.close()
