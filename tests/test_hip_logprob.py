"""Log-probabilities on the MI355X (include/zgml_hip.h: zgml_hip_logprobs and the `logprobs` field of zgml_sampling; kernels:
zgml_amd/csrc/logprob.hip).

Every comparison is bit equality of f32 words: the device's value against zgml_amd/csrc/sample.h — the same functions, compiled
for the host into tests/cpp/logprob_probe.cpp — over the same logits bits. A resident loop is compared with the same plan driven
from the host (Session.step / BatchSession.step / resident_prefill -> downloaded logits -> probe), as tests/test_hip_sample.py
does for the tokens. The batched loop's reference is the BATCHED plan driven from the host, as in tests/test_hip_sample.py: the
decode plan's M = 1 kernels agree with the batched plan's to the parity bar only, not to the bit, so the single-sequence runs are
no bit-exact reference for it."""
import ctypes as C

import numpy as np
import pytest

from zgml_amd import DeviceOp, DeviceProgram, ProgramIO, capi, llama
from tests import spec_model as SM
from tests import spec_sampled_model as SSM
from tests.test_hip_sample import FIRST, N, PARAMS, PROMPT_LEN, prompt, resident, session_behind_prompt, tiny
from tests.test_hip_spec_decode import FIRST_AT_0, _download, drafts_of, spec_session
from tests.test_logprob_host import NAN_WORD, SIZES, bits, c_logprob, c_logprobs, model, patterns, tokens_of
from tests.test_penalty_host import c_sample_penalized
from tests.test_sample_host import c_sample

pytestmark = pytest.mark.gpu
f32 = np.float32
S = capi.SamplingC.of
PEN = dict(repeat_penalty=1.3, penalty_window=16)


def upload(be, v):
    prog = DeviceProgram(ops=[DeviceOp.elementwise("abs", 1, 0, 0, 1)], buffer_sizes=[v.size, 1], initial_uploads=[ProgramIO(0, v)])
    return be.compileProgram(prog)


def same_bits(got, want):
    return np.array_equal(bits(got), bits(want))


# ── zgml_hip_logprobs on crafted vectors ───────────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("n", SIZES)
def test_logprobs_on_crafted_vectors(hip_backend, n):
    for name, v in patterns(n):
        h = upload(hip_backend, v)
        t = tokens_of(v)
        want = c_logprobs(v, t)
        got = np.array([hip_backend.logprobs(h, 0, 0, n, [tok])[0] for tok in t], f32)  # rows = 1
        assert not hip_backend.last_error(), hip_backend.last_error()
        assert same_bits(got, want), (name, n, got, want)
        hip_backend.freeProgram(h)


def test_logprobs_edges(hip_backend):
    for v in (np.array([0.5, -np.inf, np.nan, -2.0], f32), np.full(5000, -np.inf, f32), np.full(3, np.nan, f32), np.array([3.5], f32), np.array([-0.0], f32)):
        h = upload(hip_backend, v)
        t = list(range(min(v.size, 4))) + [v.size - 1]
        assert same_bits([hip_backend.logprobs(h, 0, 0, v.size, [tok])[0] for tok in t], c_logprobs(v, t))
        hip_backend.freeProgram(h)
    v = np.zeros(5000, f32)
    v[4500] = np.inf
    h = upload(hip_backend, v)
    assert bits(hip_backend.logprobs(h, 0, 0, v.size, [0])).tolist() == [NAN_WORD]
    hip_backend.freeProgram(h)


@pytest.mark.parametrize("n", [3000, 4097])
def test_rows_that_straddle_block_and_alignment_boundaries(hip_backend, n):
    """rows = 3 at offset 1001: the rows start at elements 1001, 1001 + n, 1001 + 2 n of the buffer, which no 16-byte load may
    assume aligned (n = 4097: every row at another misalignment), and a row's blocks are counted from the row's own start"""
    rng = np.random.default_rng(n)
    v = (3.0 * rng.standard_normal(1001 + 3 * n + 7)).astype(f32)
    v[1001 + n + n - 1] = 12.0  # row 1: the maximum at its last element
    h = upload(hip_backend, v)
    for toks in ([0, n - 1, n // 2], [n - 1, 4095 % n, 0], [2999, 1, n - 2]):
        got = hip_backend.logprobs(h, 0, 1001, n, toks)
        want = [c_logprob(v[1001 + i * n:1001 + (i + 1) * n], toks[i]) for i in range(3)]
        assert same_bits(got, want), (n, toks)
    assert not hip_backend.last_error(), hip_backend.last_error()
    hip_backend.freeProgram(h)


def test_logprobs_refusals(hip_backend):
    hip = capi.load_hip()
    big = (1 << 20) + 8
    v = np.random.default_rng(1).standard_normal(big).astype(f32)
    h = upload(hip_backend, v)
    u32p, fp = C.POINTER(C.c_uint32), C.POINTER(C.c_float)

    def call(buf, off, n, rows, toks=(0, 1, 2), tok_null=False, out_null=False):
        t = np.array(toks, np.uint32)
        out = np.full(max(rows, 1), 7.0, f32)
        rc = hip.zgml_hip_logprobs(hip_backend.ctx, h, buf, off, n, rows, None if tok_null else t.ctypes.data_as(u32p), None if out_null else out.ctypes.data_as(fp))
        err = hip_backend.last_error()
        hip.zgml_hip_clear_error(hip_backend.ctx)
        return rc, err, out

    for kw, text in [(dict(buf=0, off=0, n=0, rows=3), "2^20"), (dict(buf=0, off=0, n=(1 << 20) + 1, rows=1), "2^20"), (dict(buf=0, off=0, n=10, rows=0), "rows"),
                     (dict(buf=0, off=0, n=10, rows=3, toks=(0, 10, 2)), "token out of range"), (dict(buf=0, off=big - 29, n=10, rows=3), "inside the buffer"),
                     (dict(buf=0, off=big + 1, n=10, rows=1), "inside the buffer"), (dict(buf=9, off=0, n=10, rows=1), "inside the buffer"),
                     (dict(buf=0, off=0, n=10, rows=3, tok_null=True), "NULL"), (dict(buf=0, off=0, n=10, rows=3, out_null=True), "NULL")]:
        rc, err, out = call(**kw)
        assert rc == -1 and text in err, (kw, err)
        assert np.all(out == 7.0)  # nothing came back
    # the limits themselves are served, and the next call works
    rc, err, out = call(0, big - 30, 10, 3)
    assert rc == 0 and not err and same_bits(out, [c_logprob(v[big - 30 + 10 * i:big - 20 + 10 * i], i) for i in range(3)])
    got = hip_backend.logprobs(h, 0, 0, 1 << 20, [12345])
    assert same_bits(got, [c_logprob(v[:1 << 20], 12345)])
    hip_backend.freeProgram(h)


# ── zgml_hip_sample with the field ─────────────────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("n", [1, 257, 4097, 50001])
def test_sample_with_the_field(hip_backend, n):
    v = (2.0 * np.random.default_rng(n).standard_normal(n)).astype(f32)
    h = upload(hip_backend, v)
    for kw in (dict(temperature=0.8, top_k=40, top_p=0.95), dict(temperature=1.5, top_k=256, top_p=1.0), dict(**PARAMS["k40_p95"], recent=[0, n - 1, n // 2] * 3, **PEN)):
        sp = S(seed=n, stream=3, **kw)
        for pos in range(16):
            tok, cand = hip_backend.sample(h, 0, 0, n, sp, pos)
            tok2, cand2, lp = hip_backend.sample(h, 0, 0, n, sp, pos, logprobs=True)
            assert (tok2, cand2) == (tok, cand)
            assert same_bits([lp], [c_logprob(v, tok)]), (n, pos)  # (over the raw row, also with penalties)
    assert not hip_backend.last_error(), hip_backend.last_error()
    hip_backend.freeProgram(h)


# ── the single-sequence loop against the host-driven loop on the same plan ─────────────────────────────────────────────

_host = {}


def host_loop(be, kw, pen=None, first=FIRST, start=PROMPT_LEN, n=N):
    """the reference: the decode plan stepped through the vtable, every token sampled on the host from the downloaded logits by the
    header's own functions and its log-probability taken over the same row, raw. With penalties (`pen`) the window is the first
    token and every token emitted (nothing known before `start`). -> (tokens, float32 values). Computed once per case."""
    key = (tuple(sorted(kw.items())), tuple(sorted((pen or {}).items())), first, start, n)
    if key not in _host:
        sp = S(**kw, **(pen or {}))
        s, m = session_behind_prompt(be, tiny(), start)
        tok, out, lps, known = first, [], [], [first]
        for pos in range(start, start + n):
            _, logits = s.step(tok, pos)
            tok = c_sample_penalized(logits, sp, pos, known) if pen else c_sample(logits, sp, pos)
            known.append(tok)
            out.append(tok)
            lps.append(c_logprob(logits, tok))
        s.close(), m.close()
        _host[key] = (out, np.array(lps, f32))
    return list(_host[key][0]), _host[key][1].copy()


@pytest.mark.parametrize("name", list(PARAMS))
def test_resident_loop_values_equal_the_host_loop(hip_backend, name):
    kw = dict(seed=1234, stream=0, **PARAMS[name])
    want, want_lp = host_loop(hip_backend, kw)
    s, m = resident(hip_backend)
    plain, _ = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**kw))
    got, produced, lp = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**kw), logprobs=True)
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert got.tolist() == plain.tolist() == want and produced == N
    assert same_bits(lp, want_lp), (lp, want_lp)
    assert np.all(lp <= 0) and np.all(np.isfinite(lp))
    # with a repetition penalty the stream changes, and the value is still the one over the RAW row
    pen_want, pen_lp = host_loop(hip_backend, kw, PEN)
    got, produced, lp = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**kw, **PEN), logprobs=True)
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert got.tolist() == pen_want and produced == N and same_bits(lp, pen_lp)
    if name != "k1":
        assert pen_want != want  # precondition: the penalty does something
    s.close(), m.close()


def test_stop_token_and_continuation(hip_backend):
    kw = dict(seed=3, stream=0, **PARAMS["k256_p1"])
    want, want_lp = host_loop(hip_backend, kw)
    at = next(i for i in range(3, N - 2) if want[i] not in want[:i])  # a stop token the unstopped stream emits first at an index >= 3
    s, m = resident(hip_backend)
    got, produced, lp = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(stop=[want[at]], **kw), logprobs=True)
    assert produced == at + 1 and got[:at + 1].tolist() == want[:at + 1] and np.all(got[at + 1:] == -1)
    assert same_bits(lp[:at + 1], want_lp[:at + 1])  # the stop token's own entry is its row's value ...
    assert bits(lp[at + 1:]).tolist() == [NAN_WORD] * (N - at - 1)  # ... and no frozen step wrote behind it
    # continuing from the stop gives the rest of the uninterrupted call's values
    rest, n2, lp2 = s.resident_decode_sampled(want[at], PROMPT_LEN + at + 1, N - at - 1, S(**kw), logprobs=True)
    assert n2 == N - at - 1 and rest.tolist() == want[at + 1:] and same_bits(lp2, want_lp[at + 1:])
    assert not hip_backend.last_error(), hip_backend.last_error()
    s.close(), m.close()


def test_calls_alternate_on_one_program(hip_backend):
    kw = dict(seed=77, stream=0, **PARAMS["k40_p95"])
    want, want_lp = host_loop(hip_backend, kw)
    pen_want, pen_lp = host_loop(hip_backend, kw, PEN)
    s, m = resident(hip_backend)
    first, _ = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**kw))
    a, _, lp_a = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**kw), logprobs=True)
    b, _, lp_b = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**kw, **PEN), logprobs=True)
    last, _ = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**kw))
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert first.tolist() == last.tolist() == a.tolist() == want and b.tolist() == pen_want
    assert same_bits(lp_a, want_lp) and same_bits(lp_b, pen_lp)
    s.close(), m.close()


def test_logprobs_result_hands_out_the_last_call_with_the_word(hip_backend):
    hip, fp = capi.load_hip(), C.POINTER(C.c_float)
    kw = dict(seed=1234, stream=0, **PARAMS["k40_p95"])
    _, want_lp = host_loop(hip_backend, kw)
    s, m = resident(hip_backend)
    _, _, lp = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**kw), logprobs=True)
    assert same_bits(lp, want_lp)
    s.resident_decode_sampled(FIRST, PROMPT_LEN, 5, S(**kw))  # a call without the word leaves the values as they are
    few, more = np.full(4, 7.0, f32), np.full(N + 3, 7.0, f32)
    assert hip.zgml_hip_logprobs_result(hip_backend.ctx, few.ctypes.data_as(fp), 4) == N and same_bits(few, want_lp[:4])
    assert hip.zgml_hip_logprobs_result(hip_backend.ctx, more.ctypes.data_as(fp), N + 3) == N
    assert same_bits(more[:N], want_lp) and np.all(more[N:] == 7.0)
    assert hip.zgml_hip_logprobs_result(hip_backend.ctx, None, 0) == N and not hip_backend.last_error()
    assert hip.zgml_hip_logprobs_result(hip_backend.ctx, None, 2) == -1 and "NULL" in hip_backend.last_error()
    hip.zgml_hip_clear_error(hip_backend.ctx)
    s.close(), m.close()


# ── batched ────────────────────────────────────────────────────────────────────────────────────────────────────────────

def test_batched_values_equal_the_host_driven_batched_plan(hip_backend):
    """B = 3, counts 24 / 5 / 0 from position 0; sequence 1 without the field beside two with it; sequence 0 stopped early in a
    second call. The reference is the same batched plan stepped through the vtable, each row sampled and scored on the host."""
    cfg, B = tiny(), 3
    firsts, steps = [90, 292, 22], [24, 5, 0]
    kws = [dict(seed=5, stream=0, **PARAMS["k40_p95"]), dict(seed=5, stream=1, **PARAMS["k256_p1"]), dict(seed=9, stream=2, **PARAMS["k40_p95"])]
    sps = [S(**kw) for kw in kws]
    bm = llama.BatchModel(cfg, B)
    host = llama.BatchSession(bm, llama.hip_backend_fns(hip_backend), B)
    tok, pos, want, want_lp = list(firsts), [0] * B, [[] for _ in range(B)], [[] for _ in range(B)]
    for i in range(max(steps)):
        _, logits = host.step(tok, pos)  # (a sequence behind its count repeats its step, as the device loop's does)
        for b in range(B):
            if i < steps[b]:
                tok[b] = c_sample(logits[b], sps[b], pos[b])
                pos[b] += 1
                want[b].append(tok[b])
                want_lp[b].append(c_logprob(logits[b], tok[b]))
    host.close()
    dev = llama.BatchSession(bm, llama.hip_backend_fns(hip_backend), B)
    dev.resident_setup(hip_backend)
    plain, _ = dev.resident_decode_batch_sampled(firsts, [0] * B, steps, sps)
    got, produced, lp = dev.resident_decode_batch_sampled(firsts, [0] * B, steps, sps, logprobs=[True, False, True])
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert produced.tolist() == steps and np.array_equal(got, plain)
    for b in range(B):
        assert got[b, :steps[b]].tolist() == want[b], b
    assert same_bits(lp[0], want_lp[0])
    assert bits(lp[1]).tolist() == [NAN_WORD] * 24 and bits(lp[2]).tolist() == [NAN_WORD] * 24  # the field off; a count of 0
    got, produced, lp = dev.resident_decode_batch_sampled(firsts, [0] * B, steps, sps, logprobs=True)
    assert same_bits(lp[1, :5], want_lp[1]) and bits(lp[1, 5:]).tolist() == [NAN_WORD] * 19  # behind the count: frozen steps write nothing
    # sequence 0 stopped early: its stop token's entry, then the NaN; the others as before
    at = next(i for i in range(3, 20) if want[0][i] not in want[0][:i])
    stopped = [S(stop=[want[0][at]], **kws[0]), sps[1], sps[2]]
    got, produced, lp = dev.resident_decode_batch_sampled(firsts, [0] * B, steps, stopped, logprobs=True)
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert produced.tolist() == [at + 1, 5, 0]
    assert same_bits(lp[0, :at + 1], want_lp[0][:at + 1]) and bits(lp[0, at + 1:]).tolist() == [NAN_WORD] * (23 - at)
    assert same_bits(lp[1, :5], want_lp[1])
    for x in (dev, bm):
        x.close()


# ── speculative ────────────────────────────────────────────────────────────────────────────────────────────────────────

def spec_host(be, s, m, sp, first, start, n, T, drafts, stop=()):
    """The verify loop of the contract driven from the host on the same plan: zgml_hip_resident_prefill of the step's candidates,
    the T logits rows downloaded, every row sampled and scored by the header. -> (tokens, values, n_produced)"""
    V = m.cfg.vocab_size
    hist, pos, out, lps, stopped = [first], start, [], [], False
    while len(out) < n and not stopped:
        if drafts is not None:
            c, _ = SM.candidates_provided(hist[-1], pos, start, drafts, T)
        else:
            c, _ = SM.candidates_lookup(hist, pos - start, T, 2)
        s.resident_prefill(c, pos)
        rows = _download(be, s.handle, m.buf("logits"), T * V).reshape(T, V)
        g = [c_sample(rows[j], sp, pos + j) for j in range(T)]
        k, stopped = SSM.stop_cut(g, min(SM.accept(c, g) + 1, n - len(out)), set(stop))
        out += g[:k]
        lps += [c_logprob(rows[j], g[j]) for j in range(k)]
        hist += g[:k]
        pos += k
    return out, np.array(lps, f32), len(out)


@pytest.mark.parametrize("form", ["perfect", "wrong_everywhere", "ngram"])
def test_speculative_values(hip_backend, form):
    """T = 3, 23 tokens: not a multiple of T, so the last step is cut"""
    cfg, T, n = tiny(), 3, 23
    kw = dict(seed=1234, stream=0, **PARAMS["k40_p95"])
    s, m = spec_session(hip_backend, cfg, T)
    stream, _, _ = spec_host(hip_backend, s, m, S(**kw), FIRST_AT_0, 0, n + T - 1, T, drafts=[])
    drafts = drafts_of(form, stream, cfg.vocab_size)
    want, want_lp, _ = spec_host(hip_backend, s, m, S(**kw), FIRST_AT_0, 0, n, T, drafts)
    plain, _, stats0 = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, n, S(**kw), drafts=drafts)
    got, produced, stats, lp = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, n, S(**kw), drafts=drafts, logprobs=True)
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert got.tolist() == plain.tolist() == want and produced == n and stats == stats0
    assert same_bits(lp, want_lp), (form, lp, want_lp)
    if form == "perfect":
        assert stats["steps"] == -(-n // T)  # precondition: steps emit several tokens, the last one is cut
    s.close(), m.close()


def test_speculative_stop_token_inside_a_step(hip_backend):
    cfg, T, n = tiny(), 3, 23
    kw = dict(seed=1234, stream=0, **PARAMS["k40_p95"])
    s, m = spec_session(hip_backend, cfg, T)
    stream, _, _ = spec_host(hip_backend, s, m, S(**kw), FIRST_AT_0, 0, n + T - 1, T, drafts=[])
    at = next(i for i in range(3, n - 2) if i % T == 1 and stream[i] not in stream[:i])  # with perfect drafts: the middle row of a step
    want, want_lp, made = spec_host(hip_backend, s, m, S(**kw), FIRST_AT_0, 0, n, T, stream, stop=[stream[at]])
    assert made < n and want[-1] == stream[at]  # precondition: the stop fires inside the call
    got, produced, _, lp = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, n, S(stop=[stream[at]], **kw), drafts=stream, logprobs=True)
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert produced == made and got[:made].tolist() == want and np.all(got[made:] == -1)
    assert same_bits(lp[:made], want_lp) and bits(lp[made:]).tolist() == [NAN_WORD] * (n - made)
    # greedy speculative calls on the same program run what they ran
    g1, st1 = s.resident_decode_speculative(FIRST_AT_0, 0, n)
    k1, _, st2 = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, n, S(seed=1, **PARAMS["k1"]))
    assert g1.tolist() == k1.tolist() and st1 == st2
    s.close(), m.close()


# ── scoring a prompt ───────────────────────────────────────────────────────────────────────────────────────────────────

def test_scoring_a_prefilled_chunk(hip_backend):
    """zgml_hip_resident_prefill of an 8-token chunk at position 0, then zgml_hip_logprobs over rows 0..6 with the prompt's next
    tokens: the log-likelihood of the prompt's tokens 1..7"""
    cfg, T = tiny(), 8
    V, p = cfg.vocab_size, prompt(cfg, T)
    s, m = spec_session(hip_backend, cfg, T)
    s.resident_prefill(p, 0)
    got = hip_backend.logprobs(s.handle, m.buf("logits"), 0, V, p[1:])
    rows = _download(hip_backend, s.handle, m.buf("logits"), T * V).reshape(T, V)
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert same_bits(got, [c_logprob(rows[i], p[i + 1]) for i in range(T - 1)])
    exact = np.array([model(rows[i], [p[i + 1]])[0][0] for i in range(T - 1)])
    dist = np.array([model(rows[i], [p[i + 1]])[1][0] for i in range(T - 1)])
    assert abs(got.astype(np.float64).mean() - exact.mean()) <= (1e-5 + 2.4e-7 * np.abs(dist)).mean()  # the perplexity's exponent, under the CPU bar
    s.close(), m.close()
