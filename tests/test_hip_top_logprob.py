"""GPU tests of the alternatives (include/zgml_hip.h: the `top_logprobs` word of zgml_sampling, zgml_hip_top_logprobs,
zgml_hip_top_logprobs_result; kernel: zgml_amd/csrc/top_logprob.hip). Every comparison is bit equality against
tests/cpp/top_logprob_probe.cpp — zgml_amd/csrc/sample.h under g++ — over the same logits bits: the tokens are the candidate order
over the RAW row, the values what zgml_hip_logprobs returns for them. The loops' references are the same plans driven from the
host (Session.step / BatchSession.step / resident_prefill -> downloaded logits -> probe), as tests/test_hip_logprob.py does it."""
import ctypes as C

import numpy as np
import pytest

from zgml_amd import capi, llama
from tests import spec_model as SM
from tests.test_hip_logprob import PEN, S, same_bits, upload
from tests.test_hip_sample import FIRST, N, PARAMS, PROMPT_LEN, resident, session_behind_prompt, tiny
from tests.test_hip_spec_decode import FIRST_AT_0, _download, spec_session
from tests.test_logprob_host import NAN_WORD, bits, c_logprob
from tests.test_penalty_host import c_sample_penalized
from tests.test_sample_host import c_sample
from tests.test_top_logprob_host import COUNTS, c_top, edge_rows, rows_of

pytestmark = pytest.mark.gpu
f32 = np.float32


def same_top(got, want):
    """(tokens, values) against (tokens, values): the tokens equal, the values by bits"""
    return np.array_equal(np.asarray(got[0]), np.asarray(want[0])) and same_bits(got[1], want[1])


def padding(alt, val):
    return np.all(np.asarray(alt) == -1) and np.all(bits(val) == NAN_WORD)


def c_tops(rows, a, width=None):
    """the probe's alternatives of several rows: (int64[rows, width], float32[rows, width])"""
    pairs = [c_top(v, a, width) for v in rows]
    return np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs], f32)


# ── 1. zgml_hip_top_logprobs on crafted rows ───────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("n", [1, 64, 65, 257, 1793, 4097, 57345])
def test_top_logprobs_on_crafted_rows(hip_backend, n):
    for name, v in rows_of(n) + edge_rows(n):
        h = upload(hip_backend, v)
        for a in COUNTS:
            alt, val = hip_backend.top_logprobs(h, 0, 0, n, 1, a)
            assert same_top((alt[0], val[0]), c_top(v, a)), (name, n, a, alt, val)
            ae = min(a, n)
            if a == 64:  # every value is Backend.logprobs of its token on the same row
                assert same_bits(val[0, :ae], [hip_backend.logprobs(h, 0, 0, n, [int(t)])[0] for t in alt[0, :ae]]), (name, n, a)
        assert not hip_backend.last_error(), hip_backend.last_error()
        hip_backend.freeProgram(h)


@pytest.mark.parametrize("n", [3000, 4097])
def test_rows_at_three_misalignments(hip_backend, n):
    """rows = 3 at offset 1001: no 16-byte load may assume a row aligned, and a row's blocks and slices — and the indices in its
    keys — are counted from the row's own start"""
    rng = np.random.default_rng(n)
    v = (3.0 * rng.standard_normal(1001 + 3 * n + 7)).astype(f32)
    v[1001 + n + n - 1] = 12.0  # row 1: the maximum at its last element
    v[1001 + 2 * n] = 13.0  # row 2: at its first
    h = upload(hip_backend, v)
    rows = [v[1001 + i * n:1001 + (i + 1) * n] for i in range(3)]
    for a in COUNTS:
        got = hip_backend.top_logprobs(h, 0, 1001, n, 3, a)
        assert same_top(got, c_tops(rows, a)), (n, a)
        assert got[0][1, 0] == n - 1 and got[0][2, 0] == 0
        assert same_bits(got[1][:, 0], hip_backend.logprobs(h, 0, 1001, n, got[0][:, 0]))
    assert not hip_backend.last_error(), hip_backend.last_error()
    hip_backend.freeProgram(h)


# ── 2. refusals ────────────────────────────────────────────────────────────────────────────────────────────────────────

def test_top_logprobs_refusals(hip_backend):
    hip = capi.load_hip()
    big = (1 << 20) + 8
    v = np.random.default_rng(1).standard_normal(big).astype(f32)
    h = upload(hip_backend, v)

    def call(buf, off, n, rows, top_n, tok_null=False, out_null=False):
        tok, out = np.full(max(rows, 1) * 64, 7, np.int64), np.full(max(rows, 1) * 64, 7.0, f32)
        rc = hip.zgml_hip_top_logprobs(hip_backend.ctx, h, buf, off, n, rows, top_n, None if tok_null else tok.ctypes.data_as(C.POINTER(C.c_int64)),
                                       None if out_null else out.ctypes.data_as(C.POINTER(C.c_float)))
        err = hip_backend.last_error()
        hip.zgml_hip_clear_error(hip_backend.ctx)
        return rc, err, tok, out

    for kw, text in [(dict(buf=0, off=0, n=0, rows=3, top_n=5), "2^20"), (dict(buf=0, off=0, n=(1 << 20) + 1, rows=1, top_n=5), "2^20"),
                     (dict(buf=0, off=0, n=10, rows=0, top_n=5), "rows"), (dict(buf=0, off=big - 29, n=10, rows=3, top_n=5), "inside the buffer"),
                     (dict(buf=0, off=big + 1, n=10, rows=1, top_n=5), "inside the buffer"), (dict(buf=9, off=0, n=10, rows=1, top_n=5), "inside the buffer"),
                     (dict(buf=0, off=0, n=10, rows=3, top_n=5, tok_null=True), "NULL"), (dict(buf=0, off=0, n=10, rows=3, top_n=5, out_null=True), "NULL"),
                     (dict(buf=0, off=0, n=10, rows=3, top_n=0), "top_n"), (dict(buf=0, off=0, n=10, rows=3, top_n=65), "top_n")]:
        rc, err, tok, out = call(**kw)
        assert rc == -1 and text in err, (kw, err)
        assert np.all(tok == 7) and np.all(out == 7.0)  # nothing came back
    # the limits themselves are served, and the next call works
    rc, err, tok, out = call(0, big - 30, 10, 3, 64)
    want = c_tops([v[big - 30 + 10 * i:big - 20 + 10 * i] for i in range(3)], 64)
    assert rc == 0 and not err and same_top((tok[:192].reshape(3, 64), out[:192].reshape(3, 64)), want)
    assert same_top(hip_backend.top_logprobs(h, 0, 0, 1 << 20, 1, 64), c_tops([v[:1 << 20]], 64))
    hip_backend.freeProgram(h)


# ── 3. zgml_hip_sample ─────────────────────────────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("n", [1, 257, 4097, 50001])
def test_sample_with_the_word(hip_backend, n):
    v = (2.0 * np.random.default_rng(n).standard_normal(n)).astype(f32)
    h = upload(hip_backend, v)
    want = c_top(v, 5, min(5, n))
    for kw in (dict(temperature=0.8, top_k=40, top_p=0.95), dict(temperature=1.5, top_k=256, top_p=1.0), dict(**PARAMS["k40_p95"], recent=[0, n - 1, n // 2] * 3, **PEN)):
        sp = S(seed=n, stream=3, **kw)
        for pos in range(8):
            tok, cand = hip_backend.sample(h, 0, 0, n, sp, pos)
            tok2, cand2, lp, alt, val = hip_backend.sample(h, 0, 0, n, sp, pos, top_logprobs=5)
            assert (tok2, cand2) == (tok, cand)  # the token and the candidates are unchanged
            assert same_bits([lp], [c_logprob(v, tok)]) and same_top((alt, val), want), (n, pos, kw)
            if "recent" not in kw:
                assert alt.tolist() == cand[:5]  # without penalties: the pick's first candidates
    assert not hip_backend.last_error(), hip_backend.last_error()
    hip_backend.freeProgram(h)


def test_sample_under_penalties_reads_the_raw_row(hip_backend):
    """the maximum 5.0 at a token listed in `recent`, the rest below 4.5, repeat_penalty = 2: the penalised pick ranks that token
    at 2.5, behind others, while alternative 0 — over the raw row — is that token"""
    n, at = 4097, 3000
    v = np.random.default_rng(5).uniform(-1.0, 4.4, n).astype(f32)
    v[at] = 5.0
    h = upload(hip_backend, v)
    sp = S(temperature=1.0, top_k=40, top_p=1.0, seed=2, recent=[at], repeat_penalty=2.0, penalty_window=4)
    tok, cand, lp, alt, val = hip_backend.sample(h, 0, 0, n, sp, 0, top_logprobs=5)
    assert alt[0] == at and cand[0] != at and cand[0] == int(np.argmax(np.where(np.arange(n) == at, -np.inf, v)))
    assert same_top((alt, val), c_top(v, 5))
    assert not hip_backend.last_error(), hip_backend.last_error()
    hip_backend.freeProgram(h)


# ── 4. the single-sequence loop against the host-driven loop on the same plan ──────────────────────────────────────────

_host = {}


def host_loop(be, kw, pen=None, first=FIRST, start=PROMPT_LEN, n=N):
    """the reference: the decode plan stepped through the vtable, every token sampled on the host from the downloaded logits by the
    header's own functions; the rows are kept. -> (tokens, float32 values, the logits rows). Computed once per case."""
    key = (tuple(sorted(kw.items())), tuple(sorted((pen or {}).items())), first, start, n)
    if key not in _host:
        sp = S(**kw, **(pen or {}))
        s, m = session_behind_prompt(be, tiny(), start)
        tok, out, lps, rows, known = first, [], [], [], [first]
        for pos in range(start, start + n):
            _, logits = s.step(tok, pos)
            tok = c_sample_penalized(logits, sp, pos, known) if pen else c_sample(logits, sp, pos)
            known.append(tok)
            out.append(tok)
            lps.append(c_logprob(logits, tok))
            rows.append(np.array(logits, f32))
        s.close(), m.close()
        _host[key] = (out, np.array(lps, f32), rows)
    return list(_host[key][0]), _host[key][1].copy(), _host[key][2]


@pytest.mark.parametrize("a", [5, 64])
def test_resident_loop_alternatives_equal_the_host_loop(hip_backend, a):
    kw = dict(seed=1234, stream=0, **PARAMS["k40_p95"])
    s, m = resident(hip_backend)
    for pen in (None, PEN):
        want, want_lp, rows = host_loop(hip_backend, kw, pen)
        sp = S(**kw, **(pen or {}))
        plain, _, lp0 = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, sp, logprobs=True)
        got, produced, lp, top = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, sp, top_logprobs=a)
        assert not hip_backend.last_error(), hip_backend.last_error()
        assert got.tolist() == plain.tolist() == want and produced == N  # tokens and values: those of the run without the word
        assert same_bits(lp, lp0) and same_bits(lp, want_lp)
        assert top[0].shape == (N, a) and same_top(top, c_tops(rows, a)), (a, pen)
    s.close(), m.close()


def test_stop_token_and_continuation(hip_backend):
    kw = dict(seed=3, stream=0, **PARAMS["k256_p1"])
    want, want_lp, rows = host_loop(hip_backend, kw)
    all_top = c_tops(rows, 5)
    at = next(i for i in range(3, N - 2) if want[i] not in want[:i])
    s, m = resident(hip_backend)
    got, produced, lp, top = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(stop=[want[at]], **kw), top_logprobs=5)
    assert produced == at + 1 and got[:at + 1].tolist() == want[:at + 1]
    assert same_top((top[0][:at + 1], top[1][:at + 1]), (all_top[0][:at + 1], all_top[1][:at + 1]))  # the stop token's own entry ...
    assert padding(top[0][at + 1:], top[1][at + 1:])  # ... and no frozen step wrote behind it
    # two calls that continue each other equal one call
    rest, n2, lp2, top2 = s.resident_decode_sampled(want[at], PROMPT_LEN + at + 1, N - at - 1, S(**kw), top_logprobs=5)
    assert n2 == N - at - 1 and rest.tolist() == want[at + 1:] and same_top(top2, (all_top[0][at + 1:], all_top[1][at + 1:]))
    assert not hip_backend.last_error(), hip_backend.last_error()
    s.close(), m.close()


def test_calls_alternate_on_one_program(hip_backend):
    kw = dict(seed=77, stream=0, **PARAMS["k40_p95"])
    want, want_lp, rows = host_loop(hip_backend, kw)
    pen_want, pen_lp, pen_rows = host_loop(hip_backend, kw, PEN)
    s, m = resident(hip_backend)
    first, _ = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**kw))
    a, _, lp_a, top_a = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**kw), top_logprobs=5)
    b, _, lp_b, top_b = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**kw, **PEN), top_logprobs=64)
    c, _, lp_c = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**kw), logprobs=True)
    d, _, lp_d, top_d = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**kw), top_logprobs=64)  # the graph captured with a = 5 serves 64
    e, _, lp_e, top_e = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**kw, **PEN), top_logprobs=5)
    last, _ = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**kw, **PEN))
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert first.tolist() == a.tolist() == c.tolist() == d.tolist() == want and b.tolist() == e.tolist() == last.tolist() == pen_want
    assert all(same_bits(x, want_lp) for x in (lp_a, lp_c, lp_d)) and same_bits(lp_b, pen_lp) and same_bits(lp_e, pen_lp)
    assert same_top(top_a, c_tops(rows, 5)) and same_top(top_d, c_tops(rows, 64))
    assert same_top(top_b, c_tops(pen_rows, 64)) and same_top(top_e, c_tops(pen_rows, 5))
    s.close(), m.close()


def test_a_longer_call_after_the_graphs_were_captured(hip_backend):
    """3 steps in each kind, plain and penalised, capture all six graphs over a token table (and values and pairs) of capacity 3;
    N steps then grow the tables, which every one of the graphs baked: the longer calls must still equal the host loop bit for
    bit, the short ones its first 3."""
    kw = dict(seed=1234, stream=0, **PARAMS["k40_p95"])
    s, m = resident(hip_backend)
    for n in (3, N):
        for pen in (None, PEN):
            want, want_lp, rows = host_loop(hip_backend, kw, pen)
            want_top = c_tops(rows[:n], 5)
            sp = S(**kw, **(pen or {}))
            a, made_a = s.resident_decode_sampled(FIRST, PROMPT_LEN, n, sp)
            b, made_b, lp_b = s.resident_decode_sampled(FIRST, PROMPT_LEN, n, sp, logprobs=True)
            c, made_c, lp_c, top_c = s.resident_decode_sampled(FIRST, PROMPT_LEN, n, sp, top_logprobs=5)
            assert not hip_backend.last_error(), hip_backend.last_error()
            assert made_a == made_b == made_c == n and a.tolist() == b.tolist() == c.tolist() == want[:n], (pen, n)
            assert same_bits(lp_b, want_lp[:n]) and same_bits(lp_c, want_lp[:n]), (pen, n)
            assert top_c[0].shape == (n, 5) and same_top(top_c, want_top), (pen, n)
    s.close(), m.close()


# ── 7. the getter ──────────────────────────────────────────────────────────────────────────────────────────────────────

def test_the_getter(hip_backend):
    hip = capi.load_hip()
    i64p, fp = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    ctx = hip.zgml_hip_create(0)  # a context of its own: nothing has run on it
    width = C.c_uint32(9)
    assert hip.zgml_hip_top_logprobs_result(ctx, None, None, 0, C.byref(width)) == 0 and width.value == 0  # 0 before any such call
    hip.zgml_hip_destroy(ctx)
    kw = dict(seed=1234, stream=0, **PARAMS["k40_p95"])
    _, _, rows = host_loop(hip_backend, kw)
    want = c_tops(rows, 5)
    s, m = resident(hip_backend)
    _, _, _, top = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**kw), top_logprobs=5)
    assert same_top(top, want)
    s.resident_decode_sampled(FIRST, PROMPT_LEN, 5, S(**kw))  # later calls without the word leave the values standing
    s.resident_decode_sampled(FIRST, PROMPT_LEN, 5, S(**kw), logprobs=True)
    tok, val = np.full(12, 7, np.int64), np.full(12, 7.0, f32)
    assert hip.zgml_hip_top_logprobs_result(hip_backend.ctx, tok.ctypes.data_as(i64p), val.ctypes.data_as(fp), 7, C.byref(width)) == 5 * N and width.value == 5
    assert same_top((tok[:7], val[:7]), (want[0].ravel()[:7], want[1].ravel()[:7])) and np.all(tok[7:] == 7) and np.all(val[7:] == 7.0)  # a prefix
    assert hip.zgml_hip_top_logprobs_result(hip_backend.ctx, None, None, 0, None) == 5 * N and not hip_backend.last_error()
    assert hip.zgml_hip_top_logprobs_result(hip_backend.ctx, None, val.ctypes.data_as(fp), 2, None) == -1 and "NULL" in hip_backend.last_error()
    hip.zgml_hip_clear_error(hip_backend.ctx)
    s.close(), m.close()


# ── 5. batched ─────────────────────────────────────────────────────────────────────────────────────────────────────────

B_FIRSTS, B_STEPS = [90, 292, 22], [12, 5, 12]
B_KWS = [dict(seed=5, stream=0, **PARAMS["k40_p95"]), dict(seed=5, stream=1, **PARAMS["k256_p1"], **PEN), dict(seed=9, stream=2, **PARAMS["k40_p95"])]


def batched_host_plan(be):
    """B = 3, counts 12 / 5 / 12 from position 0, sequence 1 with penalties beside two without: the batched plan stepped through the
    vtable, each row sampled on the host; a sequence behind its count repeats its step. -> (every sequence's tokens, float32
    values, the logits rows). Computed once."""
    if "batched" not in _host:
        B, sps = len(B_FIRSTS), [S(**kw) for kw in B_KWS]
        bm = llama.BatchModel(tiny(), B)
        host = llama.BatchSession(bm, llama.hip_backend_fns(be), B)
        tok, pos, want, lps, rows, known = list(B_FIRSTS), [0] * B, [[] for _ in range(B)], [[] for _ in range(B)], [[] for _ in range(B)], [[t] for t in B_FIRSTS]
        for i in range(max(B_STEPS)):
            _, logits = host.step(tok, pos)
            for b in range(B):
                if i < B_STEPS[b]:
                    tok[b] = c_sample_penalized(logits[b], sps[b], pos[b], known[b]) if b == 1 else c_sample(logits[b], sps[b], pos[b])
                    pos[b] += 1
                    known[b].append(tok[b])
                    want[b].append(tok[b])
                    lps[b].append(c_logprob(logits[b], tok[b]))
                    rows[b].append(np.array(logits[b], f32))
        host.close(), bm.close()
        _host["batched"] = (want, [np.array(x, f32) for x in lps], rows)
    want, lps, rows = _host["batched"]
    return [list(w) for w in want], [x.copy() for x in lps], [list(r) for r in rows]


def test_batched_alternatives_equal_the_host_driven_batched_plan(hip_backend):
    """The reference is batched_host_plan: the same batched plan driven from the host."""
    cfg, B = tiny(), 3
    firsts, steps, kws = B_FIRSTS, B_STEPS, B_KWS
    sps = [S(**kw) for kw in kws]
    want, _, rows = batched_host_plan(hip_backend)
    bm = llama.BatchModel(cfg, B)
    dev = llama.BatchSession(bm, llama.hip_backend_fns(hip_backend), B)
    dev.resident_setup(hip_backend)
    plain, _, lp0 = dev.resident_decode_batch_sampled(firsts, [0] * B, steps, sps, logprobs=True)
    # per-sequence counts [5, 0, 64] with `logprobs` on everywhere: width 64, row 1 all padding
    got, produced, lp, (alt, val) = dev.resident_decode_batch_sampled(firsts, [0] * B, steps, sps, logprobs=True, top_logprobs=[5, 0, 64])
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert produced.tolist() == steps and np.array_equal(got, plain) and same_bits(lp, lp0)
    for b in range(B):
        assert got[b, :steps[b]].tolist() == want[b], b
    assert alt.shape == (B, 12, 64) and padding(alt[1], val[1])
    assert same_top((alt[0, :, :5], val[0, :, :5]), c_tops(rows[0], 5)) and padding(alt[0, :, 5:], val[0, :, 5:])
    assert same_top((alt[2], val[2]), c_tops(rows[2], 64))
    # the sequence with penalties asks too: the raw select for all rows; its row frozen by its count keeps its last written entries
    got, produced, lp, (alt, val) = dev.resident_decode_batch_sampled(firsts, [0] * B, steps, sps, top_logprobs=[5, 7, 0])
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert np.array_equal(got, plain) and same_bits(lp[:2], lp0[:2]) and alt.shape == (B, 12, 7)
    assert same_top((alt[0, :, :5], val[0, :, :5]), c_tops(rows[0], 5)) and padding(alt[0, :, 5:], val[0, :, 5:])
    assert same_top((alt[1, :5], val[1, :5]), c_tops(rows[1], 7)) and padding(alt[1, 5:], val[1, 5:])  # behind the count: the frozen steps wrote nothing
    assert padding(alt[2], val[2])
    # logprobs = 0 with top_logprobs = 7: the word is ignored, all padding
    odd = [capi.with_logprobs(sps[0], top=5), capi.with_logprobs(sps[1], top=7), S(**kws[2])]
    odd[1].logprobs = 0
    got, produced = dev.resident_decode_batch_sampled(firsts, [0] * B, steps, odd)
    assert np.array_equal(got, plain)
    alt, val = capi.top_logprobs_result(hip_backend.ctx, (B, 12))
    assert alt.shape == (B, 12, 5) and same_top((alt[0], val[0]), c_tops(rows[0], 5)) and padding(alt[1:], val[1:])
    for x in (dev, bm):
        x.close()


def test_a_longer_batched_call_after_the_graphs_were_captured(hip_backend):
    """as test_a_longer_call_after_the_graphs_were_captured: 3 steps per sequence in each kind, then the counts 12 / 5 / 12"""
    B = 3
    sps = [S(**kw) for kw in B_KWS]
    want, want_lp, rows = batched_host_plan(hip_backend)
    tops = [c_tops(rows[b], a) for b, a in enumerate((5, 7, 64))]
    bm = llama.BatchModel(tiny(), B)
    dev = llama.BatchSession(bm, llama.hip_backend_fns(hip_backend), B)
    dev.resident_setup(hip_backend)
    for steps in ([3] * B, B_STEPS):
        a, made_a = dev.resident_decode_batch_sampled(B_FIRSTS, [0] * B, steps, sps)
        b, made_b, lp_b = dev.resident_decode_batch_sampled(B_FIRSTS, [0] * B, steps, sps, logprobs=True)
        c, made_c, lp_c, (alt, val) = dev.resident_decode_batch_sampled(B_FIRSTS, [0] * B, steps, sps, top_logprobs=[5, 7, 64])
        assert not hip_backend.last_error(), hip_backend.last_error()
        assert made_a.tolist() == made_b.tolist() == made_c.tolist() == steps and np.array_equal(a, b) and np.array_equal(a, c)
        assert alt.shape == (B, max(steps), 64)
        for i, n in enumerate(steps):
            assert a[i, :n].tolist() == want[i][:n] and np.all(a[i, n:] == -1), (steps, i)
            assert same_bits(lp_b[i, :n], want_lp[i][:n]) and same_bits(lp_c[i, :n], want_lp[i][:n]), (steps, i)
            w = tops[i][0].shape[1]
            assert same_top((alt[i, :n, :w], val[i, :n, :w]), (tops[i][0][:n], tops[i][1][:n])), (steps, i)
            assert padding(alt[i, :n, w:], val[i, :n, w:]) and padding(alt[i, n:], val[i, n:]), (steps, i)
    for x in (dev, bm):
        x.close()


# ── 6. the sampled verify step ─────────────────────────────────────────────────────────────────────────────────────────

def replay(be, s, m, toks, start, T, drafts):
    """The verify steps of a call whose emitted tokens are `toks`, driven from the host on the same plan: the step's candidates
    through zgml_hip_resident_prefill, the T logits rows downloaded; how many tokens a step emitted follows from the candidates
    and the tokens themselves (the accepted prefix, then one more). -> the logits row that emitted each token"""
    V = m.cfg.vocab_size
    hist, pos, rows, o = [FIRST_AT_0], start, [], 0
    while o < len(toks):
        c, _ = SM.candidates_provided(hist[-1], pos, start, drafts, T)
        s.resident_prefill(c, pos)
        r = _download(be, s.handle, m.buf("logits"), T * V).reshape(T, V).copy()
        k = 0
        while True:  # row k emitted toks[o + k]; the next row counts only if its candidate was that token
            rows.append(r[k])
            k += 1
            if k == T or o + k == len(toks) or c[k] != toks[o + k - 1]:
                break
        hist += toks[o:o + k]
        pos += k
        o += k
    return rows


@pytest.mark.parametrize("pen", [None, PEN])
def test_speculative_alternatives(hip_backend, pen):
    """T = 3, 23 tokens, drafts wrong at five places: steps are partly rejected and the last one is cut"""
    cfg, T, n = tiny(), 3, 23
    kw = dict(seed=1234, stream=0, **PARAMS["k40_p95"], **(pen or {}))
    s, m = spec_session(hip_backend, cfg, T)
    stream, _, _ = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, n + T - 1, S(**kw), drafts=[])
    drafts = [int(t) for t in stream]
    for i in (4, 9, 12, 16, 19):  # (a wrong draft at the place of a step's own last token would never be a candidate)
        drafts[i] = (drafts[i] + 1) % cfg.vocab_size
    plain, _, stats0, lp0 = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, n, S(**kw), drafts=drafts, logprobs=True)
    got, produced, stats, lp, top = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, n, S(**kw), drafts=drafts, top_logprobs=5)
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert got.tolist() == plain.tolist() and produced == n and stats == stats0 and same_bits(lp, lp0)  # the top form (and the raw select) change nothing
    assert 0 < stats["accepted"] < stats["drafted"]  # precondition: partly rejected
    rows = replay(hip_backend, s, m, got.tolist(), 0, T, drafts)
    assert same_bits(lp, [c_logprob(rows[i], int(got[i])) for i in range(n)])  # precondition: the replay saw the rows the call saw
    assert same_top(top, c_tops(rows, 5)), (pen, top)
    # a stop token inside a step: the entries behind the cut are padding
    at = next(i for i in range(3, n - 2) if got[i] not in got[:i].tolist())
    cut, made, _, lp2, top2 = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, n, S(stop=[int(got[at])], **kw), drafts=drafts, top_logprobs=5)
    assert made == at + 1 and cut[:made].tolist() == got[:made].tolist()
    assert same_top((top2[0][:made], top2[1][:made]), (top[0][:made], top[1][:made])) and padding(top2[0][made:], top2[1][made:])
    assert not hip_backend.last_error(), hip_backend.last_error()
    s.close(), m.close()
