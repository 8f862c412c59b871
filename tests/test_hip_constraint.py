"""Constrained decoding on the MI355X: a token automaton masks the sampled picks on the device (include/zgml_hip.h: zgml_token_dfa,
zgml_hip_constraint_create, zgml_hip_program_set_constraint; kernel: sample_select_constrained_kernel, zgml_amd/csrc/sample.hip).

Every comparison is bit-exact token, candidate-list or state equality against zgml_amd/csrc/sample.h compiled for the host
(tests/cpp/constraint_probe.cpp) over the same logits bits, the same window and the same state: no tolerance. A resident loop is
compared with the same plan driven from the host — Session.step -> downloaded logits -> probe -> next token, the window and the
automaton's state kept in Python."""
import ctypes as C

import numpy as np
import pytest

from zgml_amd import DeviceOp, DeviceProgram, ProgramIO, capi, llama
from tests import test_hip_sample as THS
from tests.test_constraint_host import Dfa, FORBIDDEN, c_constraint_candidates, c_constraint_sample, two_class_dfa
from tests.test_hip_penalty import PEN4, window_tokens
from tests.test_hip_sample import FIRST, N, PARAMS, PROMPT_LEN, _dispatches, prompt, session_behind_prompt
from tests.test_hip_spec_decode import FIRST_AT_0, spec_session
from tests.test_sample_host import c_candidates

pytestmark = pytest.mark.gpu
f32, u16 = np.float32, np.uint16
S = capi.SamplingC.of


def hashed_classes(n, n_classes=7):
    """class_of: a hash of the index"""
    i = np.arange(n, dtype=np.uint64)
    return (((i * np.uint64(2654435761)) >> np.uint64(7)) % np.uint64(n_classes)).astype(u16)


def seeded_dfa(seed, n, n_states=5, n_classes=7, always=(), never=()):
    """a seeded automaton over hashed classes: about 40 % of the transitions forbidden, no state without an allowed class (the
    walks of these tests go on); the classes `always` are allowed in every state, the classes `never` in none"""
    rng = np.random.default_rng(seed)
    nxt = rng.integers(0, n_states, (n_states, n_classes)).astype(u16)
    nxt[rng.random((n_states, n_classes)) < 0.4] = FORBIDDEN
    for s in range(n_states):
        if np.all(nxt[s] == FORBIDDEN):
            nxt[s, s % n_classes] = (s + 1) % n_states
        for c in always:
            nxt[s, c] = (s + 1 + c) % n_states
        for c in never:
            nxt[s, c] = FORBIDDEN
    return Dfa(hashed_classes(n, n_classes), nxt)


def create(be, dfa):
    return be.constraint_create(dfa.class_of, dfa.next)


# ── 1. zgml_hip_sample on crafted vectors ──────────────────────────────────────────────────────────────────────────────

def vector_program(be, vec):
    """a program whose buffer 0 holds `vec`, with the smallest resident set-up that gives it a vocabulary of vec.size (one
    sequence, d_model 1, max_seq 1; buffer 1 stands for token_input and attn_mask): zgml_hip_sample over buffer 0 then honours a
    constraint attached to sequence 0"""
    n = vec.size
    prog = DeviceProgram(ops=[DeviceOp.elementwise("abs", 1, 0, 0, 1)], buffer_sizes=[n, 1], initial_uploads=[ProgramIO(0, vec)])
    h = be.compileProgram(prog)
    embed, tab = np.zeros(n, f32), np.zeros(1, f32)
    d = capi.ResidentLlamaC()
    d.token_embed, d.cos_table, d.sin_table = embed.ctypes.data, tab.ctypes.data, tab.ctypes.data
    d.vocab, d.d_model, d.max_seq, d.d_head = n, 1, 1, 1
    d.buf_token_input, d.buf_attn_mask, d.buf_logits, d.n_rope = 1, 1, 0, 0
    assert capi.load_hip().zgml_hip_resident_setup(be.ctx, h, C.byref(d)) == 0, be.last_error()
    return h


def walk_on_device(be, h, vec, sp_kw, recent, dfa, state, name, positions=16):
    """`positions` picks through zgml_hip_sample, candidates, token and state against the probe at every one"""
    n = vec.size
    c = create(be, dfa)
    be.set_constraint(h, 0, c, state)
    assert be.constraint_state(h, 0) == state
    for pos in range(positions):
        sp = S(recent=recent, **sp_kw)
        want_cand = c_constraint_candidates(vec, sp, recent, dfa, state)
        want_tok, after = c_constraint_sample(vec, sp, pos, recent, dfa, state)
        tok, cand = be.sample(h, 0, 0, n, sp, pos)
        assert cand == want_cand, f"selection: {name} n={n} pos={pos} state={state}"
        assert tok == want_tok, f"pick: {name} n={n} pos={pos} state={state}"
        assert be.constraint_state(h, 0) == after, f"advance: {name} n={n} pos={pos}"
        state = after
    assert not be.last_error(), be.last_error()
    be.set_constraint(h, 0, None)
    assert be.constraint_state(h, 0) == -1
    be.constraint_free(c)


PEN_HARD = dict(repeat_penalty=4.0, presence_penalty=2.0, frequency_penalty=0.5, penalty_window=256)  # 6.0 becomes -1.0 or less: the allowed window tokens lose their ranks


def crafted(n, flip):
    """random logits with 6.0 — above all the rest — at token 0, token n - 1 and both sides of every slice and chunk boundary, and
    an automaton whose class 5 (allowed in every state) and class 6 (allowed in none) alternate over those tokens, `flip`
    deciding which side gets which: a boundary token wrongly dropped or wrongly kept changes the candidate list"""
    rng = np.random.default_rng(n)
    v = rng.standard_normal(n).astype(f32)
    toks, length = window_tokens(n)
    marks = sorted(set(t for t in toks if t < n))
    dfa = seeded_dfa(n + flip, n, always=(5,), never=(6,))
    for i, t in enumerate(marks):
        v[t] = 6.0
        dfa.class_of[t] = 5 if (i + flip) % 2 == 0 else 6
    if n == 1:
        dfa.class_of[0] = 5
    return v, toks, marks, dfa


@pytest.mark.parametrize("n", [1, 257, 1792, 1793, 5381, 57345])
def test_sample_on_crafted_vectors(hip_backend, n):
    be = hip_backend
    for flip in (0, 1):
        v, toks, marks, dfa = crafted(n, flip)
        if n == 57345:
            assert {0, 1791, 1792, 1793, 1793 + 1791, 1793 + 1792, n - 1} <= set(marks)  # slice 0's chunk boundary, slice 1's start and its chunk boundary
        h = vector_program(be, v)
        sp_kw = dict(temperature=0.8, top_k=40, top_p=0.95, seed=n, stream=1 + flip)
        if n > 1:  # precondition: the mask changes the candidates — forbidden boundary tokens leave, others move up
            assert c_constraint_candidates(v, S(**sp_kw), None, dfa, 2) != c_candidates(v, 40)
        walk_on_device(be, h, v, sp_kw, None, dfa, 2, f"mask flip={flip}")
        # penalties and the constraint together: the window holds the boundary tokens, allowed and forbidden, one of them thrice
        pen_kw = dict(sp_kw, top_k=256, top_p=1.0, temperature=1.5, **PEN_HARD)
        if n > 1:
            assert c_constraint_candidates(v, S(**pen_kw), toks, dfa, 0) != c_constraint_candidates(v, S(**dict(sp_kw, top_k=256)), None, dfa, 0)
        walk_on_device(be, h, v, pen_kw, toks, dfa, 0, f"mask + penalties flip={flip}")
        be.freeProgram(h)


def test_sample_special_automata(hip_backend):
    be, n = hip_backend, 5381
    v = np.random.default_rng(1000 + n).standard_normal(n).astype(f32)
    h = vector_program(be, v)
    order = np.argsort(-v, kind="stable")
    sp_kw = dict(temperature=0.8, top_k=40, top_p=1.0, seed=n)
    # pull-in: raw rank 300 — outside the 256 largest — is the first candidate, because everything above it is forbidden
    t = int(order[300])
    d = two_class_dfa(n, order[300:].tolist())
    assert t not in c_candidates(v, 256) and c_constraint_candidates(v, S(**sp_kw), None, d, 0)[0] == t
    walk_on_device(be, h, v, sp_kw, None, d, 0, "pull_in", positions=8)
    # k_eff = 3 < top_k: three allowed tokens, in three different slices
    three = [5, 1800, n - 1]
    d = two_class_dfa(n, three)
    assert sorted(c_constraint_candidates(v, S(**sp_kw), None, d, 0)) == three
    walk_on_device(be, h, v, dict(sp_kw, temperature=4.0), None, d, 0, "k_eff_3")
    # a single allowed token, the row's least likely one: returned whatever u is
    least = int(order[-1])
    d = two_class_dfa(n, [least])
    c = create(be, d)
    be.set_constraint(h, 0, c, 0)
    for pos in range(16):
        assert be.sample(h, 0, 0, n, S(**dict(sp_kw, top_p=0.5)), pos) == (least, [least])
    # no allowed token (state 1): -1 with an error, the state stays, and the next call works
    be.set_constraint(h, 0, c, 1)
    with pytest.raises(RuntimeError, match="allows no token"):
        be.sample(h, 0, 0, n, S(**sp_kw), 0)
    capi.load_hip().zgml_hip_clear_error(be.ctx)
    assert be.constraint_state(h, 0) == 1
    be.set_constraint(h, 0, c, 0)
    assert be.sample(h, 0, 0, n, S(**sp_kw), 0) == (least, [least])
    be.set_constraint(h, 0, None)
    be.constraint_free(c)
    # n_classes = 8192, the widest state row: classes by index, half of the transitions forbidden
    rng = np.random.default_rng(8192)
    nxt = rng.integers(0, 3, (3, 8192)).astype(u16)
    nxt[rng.random((3, 8192)) < 0.5] = FORBIDDEN
    d = Dfa((np.arange(n) % 8192).astype(u16), nxt)
    assert c_constraint_candidates(v, S(**sp_kw), None, d, 0) != c_candidates(v, 40)
    walk_on_device(be, h, v, sp_kw, None, d, 0, "classes_8192")
    # a row of another length than the automaton's vocab is sampled without it, and the state stays
    c = create(be, seeded_dfa(3, n, never=(0, 1, 2, 3)))
    be.set_constraint(h, 0, c, 4)
    assert be.sample(h, 0, 0, n - 1, S(**sp_kw), 3)[1] == c_candidates(v[:n - 1], 40) and be.constraint_state(h, 0) == 4
    assert not be.last_error(), be.last_error()
    be.freeProgram(h)  # (a program that goes detaches its sequences)
    be.constraint_free(c)
    assert not be.last_error(), be.last_error()


# ── 2. the resident loop against the host-driven loop on the same plan ─────────────────────────────────────────────────

SP = dict(seed=1234, stream=0, **PARAMS["k40_p95"])
V = 512  # the tiny preset's vocabulary (resident() holds the preset to it)
DFA_A, DFA_B = seeded_dfa(11, V), seeded_dfa(12, V)
_host = {}


def host_loop(be, sp_kw, pen, dfa, state, first=FIRST, start=PROMPT_LEN, n=N, stop=()):
    """the reference: the decode plan stepped through the vtable, every token sampled on the host from the downloaded logits by
    the header's own functions, the window and the automaton's state kept here. -> (tokens, the final state). Computed once per
    case and left unchanged."""
    key = (tuple(sorted(sp_kw.items())), tuple(sorted(pen.items())), id(dfa), state, first, start, n, tuple(stop))
    if key not in _host:
        sp = S(**sp_kw, **pen)
        s, m = session_behind_prompt(be, llama.preset("tiny", 64), start)
        known, tok, out = [first], first, []
        for pos in range(start, start + n):
            _, logits = s.step(tok, pos)
            tok, after = c_constraint_sample(logits, sp, pos, known, dfa, state)
            if tok < 0:
                break
            state = after
            known.append(tok)
            out.append(tok)
            if tok in stop:
                break
        s.close(), m.close()
        _host[key] = (out, state)
    return list(_host[key][0]), _host[key][1]


def resident(be, start=PROMPT_LEN):
    assert llama.preset("tiny", 64).vocab_size == V
    s, m = session_behind_prompt(be, llama.preset("tiny", 64), start)
    s.resident_setup(be)
    return s, m


@pytest.mark.parametrize("pen", [{}, PEN4], ids=["plain", "penalties"])
def test_resident_loop_equals_the_host_loop(hip_backend, pen):
    want, want_state = host_loop(hip_backend, SP, pen, DFA_A, 1)
    without, _ = host_loop(hip_backend, SP, pen, None, 0)
    assert len(want) == N and want != without  # the constraint does something
    assert want != host_loop(hip_backend, SP, PEN4 if not pen else {}, DFA_A, 1)[0]  # ... and so do the penalties under it
    s, m = resident(hip_backend)
    c = create(hip_backend, DFA_A)
    s.set_constraint(c, 1)
    got, produced = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**SP, **pen))
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert got.tolist() == want and produced == N and s.constraint_state() == want_state
    # top_k = 1: constrained greedy decoding
    k1 = dict(seed=0, **PARAMS["k1"])
    want1, state1 = host_loop(hip_backend, k1, {}, DFA_A, 1)
    s.set_constraint(c, 1)
    got, produced = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**k1))
    assert got.tolist() == want1 and produced == N and s.constraint_state() == state1
    s.set_constraint(None)
    s.close(), m.close()
    hip_backend.constraint_free(c)
    assert not hip_backend.last_error(), hip_backend.last_error()


def test_two_calls_equal_one_and_sample_starts_a_stream(hip_backend):
    want, want_state = host_loop(hip_backend, SP, PEN4, DFA_A, 1)
    s, m = resident(hip_backend)
    c = create(hip_backend, DFA_A)
    s.set_constraint(c, 1)
    a, na = s.resident_decode_sampled(FIRST, PROMPT_LEN, 10, S(**SP, **PEN4))
    b, nb = s.resident_decode_sampled(int(a[9]), PROMPT_LEN + 10, 14, S(recent=[FIRST] + a[:9].tolist(), **SP, **PEN4))  # the state persists
    assert (na, nb) == (10, 14) and a.tolist() + b.tolist() == want and s.constraint_state() == want_state
    # the first token through zgml_hip_sample over the logits a step left behind, the rest through the loop: no host bookkeeping
    s.set_constraint(c, 1)
    s.step(FIRST, PROMPT_LEN)
    tok, _ = hip_backend.sample(s.handle, m.buf("logits"), 0, V, S(recent=[FIRST], **SP, **PEN4), PROMPT_LEN)
    rest, nr = s.resident_decode_sampled(tok, PROMPT_LEN + 1, N - 1, S(recent=[FIRST], **SP, **PEN4))
    assert [tok] + rest.tolist() == want and nr == N - 1 and s.constraint_state() == want_state
    assert not hip_backend.last_error(), hip_backend.last_error()
    s.close(), m.close()
    hip_backend.constraint_free(c)


def test_constrained_and_unconstrained_calls_alternate_on_one_program(hip_backend):
    be = hip_backend
    want_con, _ = host_loop(be, SP, {}, DFA_A, 1)
    want_pen, _ = host_loop(be, SP, PEN4, DFA_A, 1)
    want = THS.host_loop(be, S(**SP))
    s, m = resident(be)
    c = create(be, DFA_A)
    d0 = _dispatches(be, s.handle)
    assert s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**SP))[0].tolist() == want
    d1 = _dispatches(be, s.handle)
    per_call = (d1[0] - d0[0], d1[1] - d0[1])  # an unconstrained call before any attach
    greedy = s.resident_decode(FIRST, PROMPT_LEN, N).tolist()
    for _ in range(2):
        s.set_constraint(c, 1)
        assert s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**SP))[0].tolist() == want_con
        s.set_constraint(c, 1)
        assert s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**SP, **PEN4))[0].tolist() == want_pen  # the same graph, penalties on
        s.set_constraint(None)
        before = _dispatches(be, s.handle)
        assert s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**SP))[0].tolist() == want
        after = _dispatches(be, s.handle)
        assert (after[0] - before[0], after[1] - before[1]) == per_call  # what it launched before the attach
        assert s.resident_decode(FIRST, PROMPT_LEN, N).tolist() == greedy
    assert not be.last_error(), be.last_error()
    s.close(), m.close()
    be.constraint_free(c)


def chain_dfa(n_states, vocab=V):
    """state s allows every token and leads to s + 1; the last state allows none"""
    nxt = np.full((n_states, 1), FORBIDDEN, u16)
    nxt[:-1, 0] = np.arange(1, n_states)
    return Dfa(np.zeros(vocab, u16), nxt)


def test_a_state_without_tokens_freezes_and_a_stop_token_advances(hip_backend):
    be = hip_backend
    plain = THS.host_loop(be, S(**SP))
    s, m = resident(be)
    c = create(be, chain_dfa(6))
    s.set_constraint(c, 2)  # three tokens are left in the chain
    got, produced = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(**SP))
    assert produced == 3 and got[:3].tolist() == plain[:3] and np.all(got[3:] == -1) and s.constraint_state() == 5
    got, produced = s.resident_decode_sampled(FIRST, PROMPT_LEN, 4, S(**SP))  # in the dead state from the first step on
    assert produced == 0 and np.all(got == -1) and s.constraint_state() == 5
    # a stop token is recorded and advances the state as any token does
    at = next(i for i in range(1, 4) if plain[i] not in plain[:i])
    s.set_constraint(c, 0)
    got, produced = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, S(stop=[plain[at]], **SP))
    assert produced == at + 1 and got[:at + 1].tolist() == plain[:at + 1] and np.all(got[at + 1:] == -1) and s.constraint_state() == at + 1
    assert host_loop(be, SP, {}, chain_dfa(6), 0, stop=(plain[at],)) == (plain[:at + 1], at + 1)
    assert not be.last_error(), be.last_error()
    s.close(), m.close()
    be.constraint_free(c)


# ── 3. batched ─────────────────────────────────────────────────────────────────────────────────────────────────────────

def test_batched_sequences_with_and_without_an_automaton(hip_backend):
    """B = 3 from position 0: an automaton; another automaton plus penalties; none. Against the same batched plan stepped from the
    host, and each sequence's stream against its single-sequence run on the decode plan."""
    be, cfg, B, n = hip_backend, llama.preset("tiny", 64), 3, 16
    firsts, states, dfas = [90, 292, 22], [1, 3, 0], [DFA_A, DFA_B, None]
    kws = [dict(seed=5, stream=0, **PARAMS["k40_p95"]), dict(seed=5, stream=1, **PARAMS["k256_p1"], **PEN4), dict(seed=9, stream=2, **PARAMS["k40_p95"])]
    sps = [S(**kw) for kw in kws]
    bm = llama.BatchModel(cfg, B)
    host = llama.BatchSession(bm, llama.hip_backend_fns(be), B)
    tok, st, known, want = list(firsts), list(states), [[t] for t in firsts], [[] for _ in range(B)]
    for pos in range(n):
        _, logits = host.step(tok, [pos] * B)
        for b in range(B):
            tok[b], st[b] = c_constraint_sample(logits[b], sps[b], pos, known[b], dfas[b], st[b])
            assert tok[b] >= 0
            known[b].append(tok[b])
            want[b].append(tok[b])
    host.close()
    cons = [create(be, DFA_A), create(be, DFA_B)]
    dev = llama.BatchSession(bm, llama.hip_backend_fns(be), B)
    dev.resident_setup(be)
    plain, _ = dev.resident_decode_batch_sampled(firsts, [0] * B, [n] * B, sps)
    dev.set_constraint(cons[0], states[0], seq=0)
    dev.set_constraint(cons[1], states[1], seq=1)
    got, produced = dev.resident_decode_batch_sampled(firsts, [0] * B, [n] * B, sps)
    assert not be.last_error(), be.last_error()
    assert produced.tolist() == [n] * B and got.tolist() == want
    assert [dev.constraint_state(b) for b in range(B)] == [st[0], st[1], -1]
    assert got[0].tolist() != plain[0].tolist() and got[1].tolist() != plain[1].tolist() and got[2].tolist() == plain[2].tolist()
    # each sequence alone on the decode plan
    s1, m1 = resident(be, 0)
    for b in range(B):
        s1.set_constraint(cons[b] if b < 2 else None, states[b])
        alone, _ = s1.resident_decode_sampled(firsts[b], 0, n, sps[b])
        assert alone.tolist() == want[b], b
    s1.set_constraint(None)
    # detached: the unconstrained launch and its graph, the streams from before the attach
    dev.set_constraint(None, seq=0)
    dev.set_constraint(None, seq=1)
    again, _ = dev.resident_decode_batch_sampled(firsts, [0] * B, [n] * B, sps)
    assert again.tolist() == plain.tolist() and not be.last_error()
    for x in (dev, bm, s1, m1):
        x.close()
    for c in cons:
        be.constraint_free(c)
    assert not be.last_error(), be.last_error()


# ── 4. log-probabilities and alternatives stay those of the raw row ────────────────────────────────────────────────────

def test_logprobs_and_alternatives_are_over_the_raw_rows(hip_backend):
    be, n, a = hip_backend, 12, 5
    s, m = resident(be)
    c = create(be, DFA_A)
    s.set_constraint(c, 1)
    toks, produced, lps, (alt_tok, alt_val) = s.resident_decode_sampled(FIRST, PROMPT_LEN, n, S(**SP, **PEN4), top_logprobs=a)
    assert produced == n and toks.tolist() == host_loop(be, SP, PEN4, DFA_A, 1)[0][:n]
    s.set_constraint(c, 1)
    toks2, _, lps2 = s.resident_decode_sampled(FIRST, PROMPT_LEN, n, S(**SP, **PEN4), logprobs=True)
    assert toks2.tolist() == toks.tolist() and lps2.view(np.uint32).tolist() == lps.view(np.uint32).tolist()
    # the same rows again, one step at a time through the vtable: zgml_hip_logprobs / zgml_hip_top_logprobs over the raw logits
    ref, mr = session_behind_prompt(be, llama.preset("tiny", 64), PROMPT_LEN)
    buf, tok, state, raw_first = mr.buf("logits"), FIRST, 1, 0
    for i in range(n):
        ref.step(tok, PROMPT_LEN + i)
        tok = int(toks[i])
        assert be.logprobs(ref.handle, buf, 0, V, [tok]).view(np.uint32)[0] == lps.view(np.uint32)[i], i
        rt, rv = be.top_logprobs(ref.handle, buf, 0, V, 1, a)
        assert rt[0].tolist() == alt_tok[i].tolist() and rv[0].view(np.uint32).tolist() == alt_val[i].view(np.uint32).tolist(), i
        raw_first += not DFA_A.allowed(state)[int(rt[0, 0])]  # the row's maximum, listed although the state forbids it
        state = DFA_A.advance(state, tok)
    assert raw_first > 0
    # zgml_hip_sample with the words set: the same values over the row it sampled
    s.set_constraint(c, 1)
    s.step(FIRST, PROMPT_LEN)
    got = be.sample(s.handle, m.buf("logits"), 0, V, S(recent=[FIRST], **SP, **PEN4), PROMPT_LEN, top_logprobs=a)
    assert got[0] == int(toks[0]) and np.float32(got[2]).view(np.uint32) == lps.view(np.uint32)[0]
    assert got[3].tolist() == alt_tok[0].tolist() and got[4].view(np.uint32).tolist() == alt_val[0].view(np.uint32).tolist()
    assert not be.last_error(), be.last_error()
    for x in (s, m, ref, mr):
        x.close()
    be.constraint_free(c)


# ── 5. refusals ────────────────────────────────────────────────────────────────────────────────────────────────────────

def test_refusals_enqueue_nothing_and_the_next_call_works(hip_backend):
    be, cfg = hip_backend, llama.preset("tiny", 64)
    hip = capi.load_hip()
    good = S(**SP)
    s, m = resident(be, 0)
    s4, m4 = spec_session(be, cfg, 4)
    bm = llama.BatchModel(cfg, 2)
    sb = llama.BatchSession(bm, llama.hip_backend_fns(be), 2)
    sb.resident_setup(be)
    bare, mb = session_behind_prompt(be, cfg, 0)  # no resident set-up
    greedy = s.resident_decode(FIRST, 0, N).tolist()
    greedy_b = sb.resident_decode_batch([1, 2], [0, 0], [3, 3]).tolist()
    spec4 = s4.resident_decode_speculative(FIRST_AT_0, 0, 8)[0].tolist()
    spec4s = s4.resident_decode_speculative_sampled(FIRST_AT_0, 0, 8, good)[0].tolist()
    before = {x: _dispatches(be, x.handle) for x in (s, s4, sb)}

    def refused(call, text):
        with pytest.raises(RuntimeError, match=text):
            call()
        hip.zgml_hip_clear_error(be.ctx)
        for x in (s, s4, sb):
            assert _dispatches(be, x.handle) == before[x], text

    cls, nxt = DFA_A.class_of, DFA_A.next
    # zgml_hip_constraint_create
    bad_cls = cls.copy()
    bad_cls[100] = 7
    bad_nxt = nxt.copy()
    bad_nxt[2, 3] = 5
    refused(lambda: be.constraint_create(bad_cls, nxt), "class")
    refused(lambda: be.constraint_create(cls, bad_nxt), "next state")
    refused(lambda: be.constraint_create(cls, nxt, n_states=0), "n_states")
    refused(lambda: be.constraint_create(cls, nxt, n_states=65536), "n_states")
    refused(lambda: be.constraint_create(cls, nxt, n_classes=0), "n_classes")
    refused(lambda: be.constraint_create(cls, nxt, n_classes=8193), "n_classes")
    # zgml_hip_program_set_constraint
    c = create(be, DFA_A)
    short = create(be, seeded_dfa(1, V - 1))
    refused(lambda: be.set_constraint(s.handle, 0, short, 0), "vocab")
    refused(lambda: be.set_constraint(s.handle, 1, c, 0), "seq")
    refused(lambda: be.set_constraint(sb.handle, 2, c, 0), "seq")
    refused(lambda: be.set_constraint(s.handle, 0, c, 5), "state")
    refused(lambda: be.set_constraint(bare.handle, 0, c, 0), "resident")
    assert s.constraint_state() == -1 and sb.constraint_state(1) == -1 and be.constraint_state(bare.handle, 0) == -1
    # the entry points that would ignore an attached constraint
    s.set_constraint(c, 1)
    s4.set_constraint(c, 1)
    sb.set_constraint(c, 1, seq=1)
    refused(lambda: s.resident_decode(FIRST, 0, N), "constraint is attached")
    refused(lambda: sb.resident_decode_batch([1, 2], [0, 0], [3, 3]), "constraint is attached")
    refused(lambda: s4.resident_decode_speculative(FIRST_AT_0, 0, 8), "constraint is attached")
    refused(lambda: s4.resident_decode_speculative_sampled(FIRST_AT_0, 0, 8, good), "constraint is attached")
    assert hip.zgml_hip_shard_step(be.ctx, s.handle, None, 0) == -1 and "constraint is attached" in be.last_error()
    hip.zgml_hip_clear_error(be.ctx)
    assert _dispatches(be, s.handle) == before[s]
    # free while attached
    refused(lambda: be.constraint_free(c), "still attached")
    assert (s.constraint_state(), s4.constraint_state(), sb.constraint_state(1)) == (1, 1, 1)  # nothing moved a state
    # the next valid call works, constrained ...
    got, produced = s.resident_decode_sampled(FIRST, 0, N, good)
    assert produced == N and got.tolist() == host_loop(be, SP, {}, DFA_A, 1, FIRST, 0, N)[0]
    # ... and after the detach everything is as before
    s.set_constraint(None)
    s4.set_constraint(None)
    sb.set_constraint(None, seq=1)
    assert s.resident_decode(FIRST, 0, N).tolist() == greedy
    assert sb.resident_decode_batch([1, 2], [0, 0], [3, 3]).tolist() == greedy_b
    assert s4.resident_decode_speculative(FIRST_AT_0, 0, 8)[0].tolist() == spec4
    assert s4.resident_decode_speculative_sampled(FIRST_AT_0, 0, 8, good)[0].tolist() == spec4s
    be.constraint_free(c)
    be.constraint_free(short)
    assert not be.last_error(), be.last_error()
    for x in (s, m, s4, m4, sb, bm, bare, mb):
        x.close()
