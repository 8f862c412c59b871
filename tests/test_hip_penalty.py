"""Repetition, presence and frequency penalties of seeded sampling on the MI355X (include/zgml_hip.h: the tail of zgml_sampling;
kernel: sample_select_penalized_kernel, zgml_amd/csrc/sample.hip).

Every comparison is bit-exact token (or candidate-list) equality against zgml_amd/csrc/sample.h compiled for the host
(tests/cpp/penalty_probe.cpp) over the same logits bits and the same window: no tolerance. A resident loop is compared with the
same plan driven from the host — Session.step -> downloaded logits -> probe -> next token, the window kept in a Python list —,
a verify step with a replay through zgml_hip_resident_prefill and zgml_hip_sample on the same plan."""
import numpy as np
import pytest

from zgml_amd import DeviceOp, DeviceProgram, ProgramIO, capi, llama
from tests import spec_model as SM
from tests import test_hip_sample as THS
from tests.test_hip_sample import FIRST, N, PARAMS, PROMPT_LEN, _dispatches, prompt, session_behind_prompt
from tests.test_hip_spec_decode import FIRST_AT_0, FIRST_AT_8, drafts_of, spec_session
from tests.test_penalty_host import c_candidates_penalized, c_sample_penalized
from tests.test_sample_host import c_candidates

pytestmark = pytest.mark.gpu
f32 = np.float32
S = capi.SamplingC.of

PEN4 = dict(repeat_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25, penalty_window=4)
FREQ64 = dict(frequency_penalty=0.75, penalty_window=64)
PEN256 = dict(repeat_penalty=1.2, presence_penalty=0.25, frequency_penalty=0.5, penalty_window=256)


# ── zgml_hip_sample on crafted vectors ─────────────────────────────────────────────────────────────────────────────────

CHUNK, MAX_SLICES = 1792, 32  # kSampleChunk, kSampleMaxSlices (zgml_amd/csrc/kernels.h)


def window_tokens(n):
    """0, n - 1, both sides of every slice boundary and of the chunk boundary inside every slice that has one, one token three
    times, one token >= n: at most 256 entries"""
    slices = min(MAX_SLICES, max(1, -(-n // CHUNK)))
    length = -(-n // slices)  # what launch_sample gives a slice
    want = [0, n - 1]
    for s in range(1, slices):
        want += [s * length - 1, s * length]
    for s in range(slices):
        if CHUNK < length and s * length + CHUNK < n:  # the slice walks a second chunk
            want += [s * length + CHUNK - 1, s * length + CHUNK]
    toks = [t for i, t in enumerate(want) if 0 <= t < n and t not in want[:i]]
    tripled = next(t for t in range(n // 2, n // 2 + 300) if t not in toks)
    if tripled < n:
        toks += [tripled] * 3
    toks.insert(len(toks) // 2, n + 7)  # touches no logit
    assert len(toks) <= 256
    return toks, length


def crafted(n):
    rng = np.random.default_rng(n)
    v = rng.standard_normal(n).astype(f32)
    toks, length = window_tokens(n)
    # positive (above and among the largest of the rest), negative, +0, -0 and -inf at the window's tokens; the tripled token is
    # the raw maximum, so that its three-fold penalty reorders the candidates whatever else the window holds
    values = [6.0, -1.5, 0.0, -0.0, -np.inf, 4.0]
    for i, t in enumerate(sorted(set(t for t in toks if t < n))):
        v[t] = 6.5 if toks.count(t) == 3 else values[i % len(values)]
    return v, toks, length


@pytest.mark.parametrize("n", [1, 257, 1792, 1793, 5381, 57345])
def test_sample_on_crafted_vectors(hip_backend, n):
    v, toks, length = crafted(n)
    if n == 57345:
        assert length == 1793 and {1791, 1792, 1793, 1793 + 1791, 1793 + 1792, n - 1} <= set(toks)  # slice 0's chunk boundary, slice 1's start and its chunk boundary
    cases = [("window", v, S(0.8, 40, 0.95, seed=n, stream=1, **PEN256), toks),
             ("window_k256", v, S(1.5, 256, 1.0, seed=n, stream=2, repeat_penalty=0.5, presence_penalty=-0.25, frequency_penalty=1.0, penalty_window=256), toks),
             ("last_4", v, S(0.8, 40, 0.95, seed=n, stream=3, **PEN4), toks)]
    if n >= 257:  # push-out: the raw maximum, penalised, is no longer the one candidate of top_k = 1
        w = rng_vector(n)
        top = int(np.argmax(w))
        sp = S(0.8, 1, 1.0, seed=n, repeat_penalty=4.0, penalty_window=1)
        assert c_candidates(w, 1) == [top] and c_candidates_penalized(w, sp, [top]) != [top]
        cases.append(("push_out", w, sp, [top]))
    if n >= 1792:  # pull-in: raw rank 300 — outside the 256 largest — lifted into the top 40
        w = rng_vector(n)
        t = int(np.argsort(-w, kind="stable")[300])
        sp = S(0.8, 40, 1.0, seed=n, repeat_penalty=0.5, presence_penalty=-3.0, penalty_window=2)
        assert w[t] > 0 and t not in c_candidates(w, 256) and t in c_candidates_penalized(w, sp, [t, t])
        cases.append(("pull_in", w, sp, [t, t]))
    for name, vec, sp, recent in cases:
        prog = DeviceProgram(ops=[DeviceOp.elementwise("abs", 1, 0, 0, 1)], buffer_sizes=[vec.size, 1], initial_uploads=[ProgramIO(0, vec)])
        h = hip_backend.compileProgram(prog)
        dev_sp = S(sp.temperature, sp.top_k, sp.top_p, seed=sp.seed, stream=sp.stream, repeat_penalty=sp.repeat_penalty, presence_penalty=sp.presence_penalty,
                   frequency_penalty=sp.frequency_penalty, penalty_window=sp.penalty_window, recent=recent)
        want_cand = c_candidates_penalized(vec, sp, recent)
        if name in ("window", "window_k256", "last_4") and n > 1:
            assert want_cand != c_candidates(vec, sp.top_k)  # precondition: the penalties change the candidates
        for pos in range(16):
            tok, cand = hip_backend.sample(h, 0, 0, n, dev_sp, pos)
            assert cand == want_cand, f"selection: {name} n={n} pos={pos}"
            assert tok == c_sample_penalized(vec, sp, pos, recent), f"pick: {name} n={n} pos={pos}"
        assert not hip_backend.last_error(), hip_backend.last_error()
        hip_backend.freeProgram(h)


def rng_vector(n):
    return np.random.default_rng(1000 + n).standard_normal(n).astype(f32)


# ── the resident loop against the host-driven loop on the same plan ────────────────────────────────────────────────────

_host = {}


def host_loop(be, sp_kw, pen, recent, first=FIRST, start=PROMPT_LEN, n=N, seq=64):
    """the reference: the decode plan stepped through the vtable, every token sampled on the host from the downloaded logits by
    the header's own functions, the window kept here: `recent` (None: nothing known before start), the first token, every token
    emitted. Computed once per case and left unchanged."""
    key = (tuple(sorted(sp_kw.items())), tuple(sorted(pen.items())), None if recent is None else tuple(recent), first, start, n, seq)
    if key not in _host:
        sp = S(**sp_kw, **pen)
        s, m = session_behind_prompt(be, llama.preset("tiny", seq), start)
        known = list(recent or []) + [first]  # the tokens at positions lo .. pos
        tok, out = first, []
        for pos in range(start, start + n):
            _, logits = s.step(tok, pos)
            tok = c_sample_penalized(logits, sp, pos, known)
            known.append(tok)
            out.append(tok)
        s.close(), m.close()
        _host[key] = out
    return list(_host[key])


def resident(be, start=PROMPT_LEN, seq=64):
    s, m = session_behind_prompt(be, llama.preset("tiny", seq), start)
    s.resident_setup(be)
    return s, m


SP = dict(seed=1234, stream=0, **PARAMS["k40_p95"])


@pytest.mark.parametrize("given", ["recent", "n_recent_0"])
def test_resident_loop_equals_the_host_loop(hip_backend, given):
    """W = 4 over 24 steps: the window evicts. The recent tokens given end with the first two tokens of the stream without them
    (chosen by the reference alone), so that they matter to the first picks."""
    without = host_loop(hip_backend, SP, PEN4, None)
    recent = prompt(llama.preset("tiny", 64))[:PROMPT_LEN - 2] + without[:2] if given == "recent" else None
    want = host_loop(hip_backend, SP, PEN4, recent)
    plain = THS.host_loop(hip_backend, S(**SP))
    assert want != plain  # the penalty does something
    assert given != "recent" or want != without  # ... and so do the recent tokens
    s, m = resident(hip_backend)
    got, produced = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(recent=recent, **SP, **PEN4))
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert got.tolist() == want and produced == N
    got, produced = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**SP))  # penalties off on the same program: today's stream
    assert got.tolist() == plain and produced == N
    s.close(), m.close()


def test_the_ring_passes_position_256(hip_backend):
    """max_seq 320, start 250, W = 256, 16 steps: positions 256 .. 265 reuse the ring's first slots"""
    start, n, seq = 250, 16, 320
    cfg = llama.preset("tiny", seq)
    recent = prompt(cfg, start)
    want = host_loop(hip_backend, SP, PEN256, recent, FIRST, start, n, seq)
    plain = host_loop(hip_backend, SP, {}, None, FIRST, start, n, seq)
    assert want != plain
    s, m = resident(hip_backend, start, seq)
    got, produced = s.resident_decode_sampled(FIRST, start, n, S(recent=recent, **SP, **PEN256))
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert got.tolist() == want and produced == n
    s.close(), m.close()


def test_two_calls_equal_one(hip_backend):
    recent = prompt(llama.preset("tiny", 64))
    want = host_loop(hip_backend, SP, PEN4, recent)
    s, m = resident(hip_backend)
    one, _ = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(recent=recent, **SP, **PEN4))
    a, na = s.resident_decode_sampled(FIRST, PROMPT_LEN, 10, S(recent=recent, **SP, **PEN4))
    b, nb = s.resident_decode_sampled(int(a[9]), PROMPT_LEN + 10, 14, S(recent=recent + [FIRST] + a[:9].tolist(), **SP, **PEN4))
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert (na, nb) == (10, 14) and a.tolist() + b.tolist() == one.tolist() == want
    s.close(), m.close()


# ── batched ────────────────────────────────────────────────────────────────────────────────────────────────────────────

def test_batched_sequences_equal_their_single_sequence_runs(hip_backend):
    """B = 4 from position 0: penalties off; W = 4; W = 64 with a frequency penalty alone; W = 4 with a stop token that fires. Each
    row is the stream of zgml_hip_resident_decode_sampled with the same parameters on the decode plan; the stopped sequence,
    continued with `recent` re-supplied, goes on as the uninterrupted single-sequence stream does."""
    cfg, B, n = llama.preset("tiny", 64), 4, 20
    firsts = [90, 292, 22, 131]
    kws = [dict(seed=5, stream=0, **PARAMS["k40_p95"]), dict(seed=5, stream=1, **PARAMS["k256_p1"], **PEN4),
           dict(seed=9, stream=2, **PARAMS["k40_p95"], **FREQ64), dict(seed=11, stream=3, **PARAMS["k256_p1"], **PEN4)]
    s1, m1 = resident(hip_backend, 0)
    want = [s1.resident_decode_sampled(firsts[b], 0, n, S(**kws[b]))[0].tolist() for b in range(B)]
    off = [s1.resident_decode_sampled(firsts[b], 0, n, S(**{k: v for k, v in kws[b].items() if "penalty" not in k}))[0].tolist() for b in range(B)]
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert all(want[b] != off[b] for b in (1, 2, 3)) and want[0] == off[0]  # the penalties do something to their sequences
    at = next(i for i in range(2, n - 4) if want[3][i] not in want[3][:i])  # sequence 3 stops at a token new to it
    stop = want[3][at]
    sps = [S(**kws[0]), S(**kws[1]), S(**kws[2]), S(stop=[stop], **kws[3])]
    bm = llama.BatchModel(cfg, B)
    dev = llama.BatchSession(bm, llama.hip_backend_fns(hip_backend), B)
    dev.resident_setup(hip_backend)
    got, produced = dev.resident_decode_batch_sampled(firsts, [0] * B, [n] * B, sps)
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert produced.tolist() == [n, n, n, at + 1]
    for b in range(B):
        k = int(produced[b])
        assert got[b, :k].tolist() == want[b][:k], b
        assert np.all(got[b, k:] == -1)
    # the stopped sequence goes on (the others take no step: they rewrite their column 0)
    rest = n - at - 1
    cont = [S(**kws[0]), S(**kws[1]), S(**kws[2]), S(recent=[firsts[3]] + want[3][:at], **kws[3])]
    got, produced = dev.resident_decode_batch_sampled(firsts[:3] + [stop], [0, 0, 0, at + 1], [0, 0, 0, rest], cont)
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert produced.tolist() == [0, 0, 0, rest] and got[3].tolist() == want[3][at + 1:]
    # penalties off everywhere on the same program: the unpenalised launch and its graph, today's streams
    got, _ = dev.resident_decode_batch_sampled(firsts, [0] * B, [n] * B, [S(**{k: v for k, v in kw.items() if "penalty" not in k}) for kw in kws])
    assert got.tolist() == off
    for x in (dev, bm, s1, m1):
        x.close()


# ── speculative sampled ────────────────────────────────────────────────────────────────────────────────────────────────

def spec_replay(be, s, m, sp_kw, pen, first, start, n, T, drafts, ngram=2, history=None):
    """The verify loop of the contract driven from the host on the same plan: zgml_hip_resident_prefill of the step's candidates,
    then zgml_hip_sample over every logits row with that row's window — the confirmed tokens and the candidates c[1..j].
    `history`: the tokens at positions 0 .. start - 1 (None: nothing is known before the call, lo = start).
    -> (tokens, statistics)"""
    V, buf = m.cfg.vocab_size, m.buf("logits")
    lo = 0 if history else start
    hist, pos, out = list(history or []) + [first], start, []  # the tokens at positions lo .. pos
    stats = {"steps": 0, "drafted": 0, "accepted": 0}
    while len(out) < n:
        if drafts is not None:
            c, real = SM.candidates_provided(hist[-1], pos, start, drafts, T)
        else:
            c, real = SM.candidates_lookup(hist, pos - lo, T, ngram)
        s.resident_prefill(c, pos)
        g = [be.sample(s.handle, buf, j * V, V, S(recent=hist + [int(t) for t in c[1:j + 1]], **sp_kw, **pen), pos + j)[0] for j in range(T)]
        a = SM.accept(c, g)
        k = min(a + 1, n - len(out))
        out += g[:k]
        hist += g[:k]
        pos += k
        stats["steps"] += 1
        stats["drafted"] += real
        stats["accepted"] += a
    return out, stats


@pytest.mark.parametrize("T", [2, 4])
def test_speculative_stream_is_the_same_for_three_draft_sources(hip_backend, T):
    cfg = llama.preset("tiny", 64)
    s, m = spec_session(hip_backend, cfg, T)
    n = N + T - 1
    stream, _ = spec_replay(hip_backend, s, m, SP, PEN4, FIRST_AT_0, 0, n, T, drafts=[])  # no real draft: one token per step
    plain, _ = spec_replay(hip_backend, s, m, SP, {}, FIRST_AT_0, 0, n, T, drafts=[])
    assert stream != plain  # the penalty does something
    sp = S(**SP, **PEN4)
    right, wrong = drafts_of("perfect", stream, cfg.vocab_size), drafts_of("wrong_everywhere", stream, cfg.vocab_size)
    assert all(d != t for d, t in zip(wrong, stream))
    for name, drafts in (("lookup", None), ("right", right), ("wrong", wrong)):
        want, want_stats = spec_replay(hip_backend, s, m, SP, PEN4, FIRST_AT_0, 0, N, T, drafts)
        toks, produced, stats = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, N, sp, drafts=drafts)
        assert not hip_backend.last_error(), hip_backend.last_error()
        print(T, name, stats)
        assert toks.tolist() == want and produced == N and stats == want_stats, name
        assert toks.tolist() == stream[:N], name  # the drafts decide the steps, never the tokens
        if name == "right":
            assert stats["accepted"] == stats["drafted"] == -(-N // T) * (T - 1)
        if name == "wrong":
            assert stats["accepted"] == 0 and stats["steps"] == N
    s.close(), m.close()


def test_speculative_window_reaches_into_the_history(hip_backend):
    """T = 4 from position 8 behind a prefilled prompt: the window of the first picks lies in opt->history. The history handed
    over ends with the first two tokens of the stream without a history (chosen by the reference alone), so that it matters."""
    cfg, T = llama.preset("tiny", 64), 4
    s, m = spec_session(hip_backend, cfg, T)
    p = prompt(cfg)
    for chunk in range(PROMPT_LEN // T):
        s.resident_prefill(p[chunk * T:(chunk + 1) * T], chunk * T)
    without, _ = spec_replay(hip_backend, s, m, SP, PEN4, FIRST_AT_8, PROMPT_LEN, N, T, drafts=[])
    history = p[:PROMPT_LEN - 2] + without[:2]
    sp = S(**SP, **PEN4)
    for drafts in (None, []):
        want, want_stats = spec_replay(hip_backend, s, m, SP, PEN4, FIRST_AT_8, PROMPT_LEN, N, T, drafts, history=history)
        assert want != without  # the history does something
        toks, produced, stats = s.resident_decode_speculative_sampled(FIRST_AT_8, PROMPT_LEN, N, sp, history=history, drafts=drafts)
        assert not hip_backend.last_error(), hip_backend.last_error()
        assert toks.tolist() == want and produced == N and stats == want_stats
    toks, _, _ = s.resident_decode_speculative_sampled(FIRST_AT_8, PROMPT_LEN, N, sp, drafts=[])  # ... and without it, lo = start_pos
    assert toks.tolist() == without
    s.close(), m.close()


def test_top_k_1_with_neutral_penalties_equals_the_greedy_speculative_loop(hip_backend):
    cfg, T = llama.preset("tiny", 64), 4
    s, m = spec_session(hip_backend, cfg, T)
    g_toks, g_stats = s.resident_decode_speculative(FIRST_AT_0, 0, N)
    for kw in (dict(penalty_window=4), dict(repeat_penalty=1.0, penalty_window=256)):
        toks, produced, stats = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, N, S(seed=99, stream=3, **PARAMS["k1"], **kw))
        assert toks.tolist() == g_toks.tolist() and produced == N and stats == g_stats and not hip_backend.last_error()
    s.close(), m.close()


# ── refusals ───────────────────────────────────────────────────────────────────────────────────────────────────────────

NAN, INF = float("nan"), float("inf")
BAD_PENALTIES = [(dict(repeat_penalty=1.1), "penalty_window > 0"), (dict(presence_penalty=0.5), "penalty_window > 0"), (dict(frequency_penalty=-0.5), "penalty_window > 0"),
                 (dict(penalty_window=257), "at most 256"), (dict(repeat_penalty=NAN, penalty_window=4), "finite"), (dict(repeat_penalty=INF, penalty_window=4), "finite"),
                 (dict(repeat_penalty=-0.5, penalty_window=4), "finite"), (dict(presence_penalty=NAN, penalty_window=4), "finite"),
                 (dict(frequency_penalty=-INF, penalty_window=4), "finite")]


def null_recent(n_recent=3, **kw):
    sp = S(**kw)
    sp.n_recent = n_recent
    return sp


def test_refusals_enqueue_nothing_and_the_next_call_works(hip_backend):
    cfg = llama.preset("tiny", 64)
    hip, V = capi.load_hip(), cfg.vocab_size
    good = dict(seed=1, **PARAMS["k40_p95"])
    s, m = resident(hip_backend, 0)
    s4, m4 = spec_session(hip_backend, cfg, 4)
    bm = llama.BatchModel(cfg, 2)
    sb = llama.BatchSession(bm, llama.hip_backend_fns(hip_backend), 2)
    sb.resident_setup(hip_backend)
    before = {x: _dispatches(hip_backend, x.handle) for x in (s, s4, sb)}

    def refused(call, text):
        with pytest.raises(RuntimeError, match=text):
            call()
        hip.zgml_hip_clear_error(hip_backend.ctx)
        for x in (s, s4, sb):
            assert _dispatches(hip_backend, x.handle) == before[x], text

    everywhere = BAD_PENALTIES + [(None, "without the recent tokens")]
    for kw, text in everywhere:
        sp = null_recent(**good, **PEN4) if kw is None else S(**good, **kw)
        refused(lambda: s.resident_decode_sampled(1, 4, 4, sp), text)
        refused(lambda: hip_backend.sample(s.handle, m.buf("logits"), 0, V, sp, 0), text)
        refused(lambda: s4.resident_decode_speculative_sampled(1, 0, 4, sp), text)
        refused(lambda: sb.resident_decode_batch_sampled([1, 1], [4, 4], [2, 2], [S(**good), sp]), text)
    # the loops: a recent token >= vocab, more recent tokens than positions before start_pos
    refused(lambda: s.resident_decode_sampled(1, 4, 4, S(recent=[1, V, 2], **good, **PEN4)), "recent token out of range")
    refused(lambda: s.resident_decode_sampled(1, 2, 4, S(recent=[1, 2, 3], **good, **PEN4)), "n_recent exceeds start_pos")
    refused(lambda: sb.resident_decode_batch_sampled([1, 1], [4, 4], [2, 2], [S(recent=[V], **good, **PEN4), S(**good)]), "recent token out of range")
    refused(lambda: sb.resident_decode_batch_sampled([1, 1], [4, 0], [2, 2], [S(**good), S(recent=[1], **good, **PEN4)]), "n_recent exceeds start_pos")
    # the verify step takes its tokens from opt->history
    refused(lambda: s4.resident_decode_speculative_sampled(1, 0, 4, S(recent=[], **good, **PEN4)), "recent must be NULL")
    refused(lambda: s4.resident_decode_speculative_sampled(1, 2, 4, S(recent=[1, 2], **good, **PEN4), history=[1, 2]), "recent must be NULL")
    # the next valid calls work: penalised, each against its reference
    got, produced = s.resident_decode_sampled(FIRST, 0, N, S(**good, **PEN4))
    assert produced == N and got.tolist() == host_loop(hip_backend, good, PEN4, None, FIRST, 0, N)
    toks, produced = sb.resident_decode_batch_sampled([1, 1], [0, 0], [3, 3], [S(**good, **PEN4), S(**good)])
    assert produced.tolist() == [3, 3] and np.all(toks >= 0)
    toks, produced, _ = s4.resident_decode_speculative_sampled(FIRST_AT_0, 0, 8, S(**good, **PEN4))
    assert produced == 8 and toks.tolist() == spec_replay(hip_backend, s4, m4, good, PEN4, FIRST_AT_0, 0, 8, 4, drafts=[])[0]
    assert not hip_backend.last_error(), hip_backend.last_error()
    for x in (s, m, s4, m4, sb, bm):
        x.close()


# ── neighbours ─────────────────────────────────────────────────────────────────────────────────────────────────────────

def test_greedy_sampled_and_penalised_alternate_on_one_program(hip_backend):
    want_pen, want = host_loop(hip_backend, SP, PEN4, None), THS.host_loop(hip_backend, S(**SP))
    s, m = resident(hip_backend)
    runs = []
    for _ in range(2):
        g = s.resident_decode(FIRST, PROMPT_LEN, N).tolist()
        a = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**SP))[0].tolist()
        p = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**SP, **PEN4))[0].tolist()
        runs.append((g, a, p))
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert runs[0] == runs[1] and runs[0][1] == want and runs[0][2] == want_pen
    assert runs[0][0] == THS.host_loop(hip_backend, S(seed=0, **PARAMS["k1"]))
    # a longer call regrows the token table, which frees every graph: each loop captures again and gives what it gave
    n2 = N + 8
    p2 = s.resident_decode_sampled(FIRST, PROMPT_LEN, n2, S(**SP, **PEN4))[0].tolist()
    assert p2[:N] == want_pen and s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**SP))[0].tolist() == want
    assert s.resident_decode(FIRST, PROMPT_LEN, N).tolist() == runs[0][0] and not hip_backend.last_error()
    s.close(), m.close()


def test_speculative_forms_and_prefill_alternate_on_one_program(hip_backend):
    cfg, T = llama.preset("tiny", 64), 4
    s, m = spec_session(hip_backend, cfg, T)
    chunk = prompt(cfg, T)
    want_pen, _ = spec_replay(hip_backend, s, m, SP, PEN4, FIRST_AT_0, 0, N, T, drafts=[])
    runs = []
    for _ in range(2):
        g = s.resident_decode_speculative(FIRST_AT_0, 0, N)[0].tolist()
        a = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, N, S(**SP))[0].tolist()
        f = s.resident_prefill(chunk, 0)
        p = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, N, S(**SP, **PEN4))[0].tolist()
        runs.append((g, a, f, p))
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert runs[0] == runs[1] and runs[0][3] == want_pen and runs[0][1] != want_pen
    s.close(), m.close()
