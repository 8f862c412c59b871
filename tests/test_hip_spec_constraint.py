"""Constrained speculative decode on the MI355X (zgml_hip_resident_decode_speculative_constrained): the verify rows of a
token_len = T plan walk the token automaton attached to the sequence — forced tokens are drafted for free, every row is masked by
its own state, the device state advances over the emitted tokens.

THE REFERENCE everywhere is the SAME T-plan driven from the host: Session.prefill(c, pos) through the vtable, all T logits rows
downloaded, every row picked by zgml_amd/csrc/sample.h (tests/cpp/constraint_probe.cpp: c_constraint_sample) under the state the
Python model tests/spec_constraint_model.py gave that row, and the model's loop — run with the very drafts and counts of the
device call, so the steps group the context alike and the logits are the same bits. Same kernels, same inputs: exact equality of
tokens, counts, statistics, states and log-probability bits, no tolerance.

Every precondition — the stream holds forced tokens, the free picks do sample, "wrong" drafts are wrong where meant, a dead end is
reached where meant — is asserted on the reference alone, before the device loop is asked."""
import ctypes as C

import numpy as np
import pytest

from zgml_amd import capi, llama
from tests import spec_constraint_model as SCM
from tests.test_constraint_host import Dfa, FORBIDDEN, c_constraint_candidates, c_constraint_sample
from tests.test_hip_constraint import hashed_classes, seeded_dfa
from tests.test_hip_l7dims import l7cfg
from tests.test_hip_penalty import PEN4
from tests.test_hip_sample import PARAMS
from tests.test_hip_spec_decode import FIRST_AT_0, FIRST_AT_8, FORMS, N, PROMPT_LEN, _dispatches, _download, drafts_of, prompt, spec_session, tiny
from tests.test_hip_spec_sampled import BAD_PARAMS
from tests.test_spec_constraint_host import chain_dfa, template_dfa

pytestmark = pytest.mark.gpu
S = capi.SamplingC.of
u16 = np.uint16
V = 512  # the tiny preset's vocabulary
SP = dict(seed=1234, stream=0, **PARAMS["k256_p1"])
ALL_FORMS = FORMS + ["none"]
TEMPLATE, TEMPLATE_FREE, TEMPLATE_LITS = template_dfa(V, [0, 1, 0, 3, 0, 6], seed=21)  # literal runs of 1, 3 and 6 forced tokens between free states
SEEDED = seeded_dfa(11, V)


class Host:
    """The reference side: a T-plan of its own stepped through the vtable, and what every row of every step was."""

    def __init__(self, be, cfg, T, start=0, threads=8):
        self.be, self.cfg, self.T = be, cfg, T
        self.s, self.m = spec_session(be, cfg, T, threads=threads)
        p = prompt(cfg, start)
        for at in range(0, start, T):
            self.s.prefill(p[at:at + T], at, want_logits=False)
        self.rows = {}  # position -> what the last step that computed its row saw

    def download(self):
        T, n = self.T, self.cfg.vocab_size
        return _download(self.be, self.s.handle, self.m.buf("logits"), T * n).reshape(T, n)

    def rows_fn(self, sp, dfa, values=0):
        """rows_fn of the model's loop. values = a > 0: also every picked row's log-probability and a alternatives, from
        zgml_hip_logprobs / zgml_hip_top_logprobs over the raw row where the plan left it"""
        T, n, buf = self.T, self.cfg.vocab_size, self.m.buf("logits")

        def rows(c, pos, row_state, known):
            self.s.prefill(c, pos, want_logits=False)
            logits, g = self.download(), []
            for j in range(T):
                if row_state[j] == SCM.DEAD:
                    g.append(SCM.NO_PICK)
                    continue
                recent = known + c[1:j + 1]
                tok, _ = c_constraint_sample(logits[j], sp, pos + j, recent, dfa, row_state[j])
                g.append(tok if tok >= 0 else SCM.NO_PICK)
                if tok < 0:
                    continue
                seen = {"pick": tok, "first": c_constraint_candidates(logits[j], sp, recent, dfa, row_state[j])[0], "state": row_state[j]}
                if values:
                    seen["lp"] = self.be.logprobs(self.s.handle, buf, j * n, n, [tok]).view(np.uint32)[0]
                    tt, tv = self.be.top_logprobs(self.s.handle, buf, j * n, n, 1, values)
                    seen["top"] = (tt[0].tolist(), tv[0].view(np.uint32).tolist())
                self.rows[pos + j] = seen
            return g
        return rows

    def loop(self, sp, dfa, state, first, start, n, values=0, **kw):
        self.rows = {}
        return SCM.spec_loop(self.rows_fn(sp, dfa, values), first, start, n, self.T, dfa.class_of, dfa.next, state, **kw)

    def close(self):
        self.s.close(), self.m.close()


@pytest.fixture(scope="module")
def hosts(hip_backend):
    made = {}

    def get(T, start=0):
        if (T, start) not in made:
            made[(T, start)] = Host(hip_backend, tiny(), T, start)
        return made[(T, start)]
    yield get
    for h in made.values():
        h.close()


def create(be, dfa):
    return be.constraint_create(dfa.class_of, dfa.next)


def device(be, s, c, state, first, start, n, sp, **kw):
    """one constrained call from `state` -> (tokens, produced, stats, the state afterwards)"""
    s.set_constraint(c, state)
    toks, produced, stats = s.resident_decode_speculative_constrained(first, start, n, sp, **kw)
    assert not be.last_error(), be.last_error()
    return toks.tolist(), produced, stats, s.constraint_state()


def drafts_for(form, stream, vocab):
    return [] if form == "none" else drafts_of(form, stream, vocab)


# ── 1. equals the host loop ────────────────────────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("pen", [{}, PEN4], ids=["plain", "penalties"])
@pytest.mark.parametrize("T", [2, 4, 5])
@pytest.mark.parametrize("which", ["seeded", "template"])
def test_equals_the_host_loop(hip_backend, hosts, which, T, pen):
    be, cfg, host = hip_backend, tiny(), hosts(T)
    dfa = SEEDED if which == "seeded" else TEMPLATE
    frc = SCM.forced(dfa.class_of, dfa.next)
    sp = S(**SP, **pen)
    lits = set(sum(TEMPLATE_LITS, []))
    if which == "seeded":
        assert all(f == SCM.NO_FORCED for f in frc)  # precondition: no forced state, the pass only propagates states
    else:
        assert sorted(len(r) for r in TEMPLATE_LITS) == [0, 0, 0, 1, 3, 6] and sum(f != SCM.NO_FORCED for f in frc) == 10
    stream = host.loop(sp, dfa, 1 if which == "seeded" else 0, FIRST_AT_0, 0, N + T - 1, drafts=[])[0]
    assert -1 not in stream  # precondition: the walk goes on, perfect drafts exist for the last step
    s, m = spec_session(be, cfg, T)
    c = create(be, dfa)
    state0 = 1 if which == "seeded" else 0
    for form in ALL_FORMS:
        drafts = drafts_for(form, stream, V)
        want = host.loop(sp, dfa, state0, FIRST_AT_0, 0, N, drafts=drafts)
        toks = want[0]
        assert want[1] == N
        if form == "wrong_everywhere":
            assert all(d != t for d, t in zip(drafts, toks))
        if form == "wrong_at_two":
            assert [i for i, (d, t) in enumerate(zip(drafts, toks)) if d != t] == [5, 14]
        if form == "perfect":
            assert drafts[:N] == toks and want[2]["steps"] == -(-N // T)
        if which == "template":
            assert sum(t in lits for t in toks) >= 8  # forced tokens in the stream
            free = [host.rows[p] for p in range(N) if frc[host.rows[p]["state"]] == SCM.NO_FORCED]
            assert sum(r["pick"] != r["first"] for r in free) >= 4  # the free picks do sample
            if form in ("none", "wrong_everywhere"):
                assert want[2]["steps"] < N  # forced runs are jumped over whatever the drafts say
        got = device(be, s, c, state0, FIRST_AT_0, 0, N, sp, drafts=drafts)
        print(which, T, form, got[2])
        assert got == want, form
    s.set_constraint(None)
    s.close(), m.close()
    be.constraint_free(c)
    assert not be.last_error(), be.last_error()


# ── 2. a fully forced chain ────────────────────────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("T", [2, 4, 5])
def test_a_fully_forced_chain(hip_backend, hosts, T):
    be, n_states = hip_backend, 32
    chain = [(7 * s + 1) % V for s in range(n_states)]
    nxt = np.full((n_states, V), FORBIDDEN, u16)
    for s in range(n_states):
        nxt[s, chain[s]] = (s + 1) % n_states  # a cycle of >= N states, each allowing one token
    dfa = Dfa(np.arange(V, dtype=u16), nxt)
    assert SCM.forced(dfa.class_of, dfa.next) == chain and n_states >= N
    sp = S(**SP)
    drafts = [(t + 1) % V for t in chain]  # wrong everywhere
    want = hosts(T).loop(sp, dfa, 0, FIRST_AT_0, 0, N, drafts=drafts)
    assert want[0] == chain[:N] and want[2]["steps"] == -(-N // T) and want[3] == N % n_states
    s, m = spec_session(be, tiny(), T)
    c = create(be, dfa)
    got = device(be, s, c, 0, FIRST_AT_0, 0, N, sp, drafts=drafts)
    assert got[0] == chain[:N] and got[2]["steps"] == -(-N // T) and got[2]["accepted"] == want[2]["accepted"]
    assert got == want
    assert device(be, s, c, 0, FIRST_AT_0, 0, N, sp) == hosts(T).loop(sp, dfa, 0, FIRST_AT_0, 0, N)  # ... and under n-gram lookup
    s.set_constraint(None)
    s.close(), m.close()
    be.constraint_free(c)


# ── 3. dead ends ───────────────────────────────────────────────────────────────────────────────────────────────────────

def test_dead_ends_in_the_middle_of_a_step_and_at_row_0(hip_backend, hosts):
    be, T, sp = hip_backend, 4, S(**SP)
    host = hosts(T)
    free = host.loop(sp, chain_dfa(V, 40), 0, FIRST_AT_0, 0, N, drafts=[])[0]
    dfa = chain_dfa(V, 7)  # every token is allowed, six times; state 6 allows none
    want = host.loop(sp, dfa, 0, FIRST_AT_0, 0, N, drafts=free)
    # precondition: step 1 emits 4 tokens, step 2 reaches state 6 at its row 2 and emits 2
    assert want[1:] == (6, {"steps": 2, "drafted": 6, "accepted": 5}, 6) and want[0][6:] == [-1] * (N - 6) and -1 not in want[0][:6]
    s, m = spec_session(be, tiny(), T)
    c = create(be, dfa)
    assert device(be, s, c, 0, FIRST_AT_0, 0, N, sp, drafts=free) == want
    # the same at row 0 of the first step: nothing is produced, the call returns 0, no error is on the context
    want0 = host.loop(sp, dfa, 6, FIRST_AT_0, 0, N, drafts=free)
    assert want0 == ([-1] * N, 0, {"steps": 1, "drafted": 3, "accepted": 0}, 6)
    assert device(be, s, c, 6, FIRST_AT_0, 0, N, sp, drafts=free) == want0
    assert device(be, s, c, 6, FIRST_AT_0, 0, N, sp) == host.loop(sp, dfa, 6, FIRST_AT_0, 0, N)  # ... under n-gram lookup
    # ... and the next call, from a live state, works
    assert device(be, s, c, 0, FIRST_AT_0, 0, N, sp, drafts=free) == want
    s.set_constraint(None)
    s.close(), m.close()
    be.constraint_free(c)


# ── 4. a stop token that is also a transition ──────────────────────────────────────────────────────────────────────────

def test_a_stop_token_cuts_the_step_and_advances_the_state(hip_backend, hosts):
    be, T, sp_kw = hip_backend, 4, dict(SP)
    host = hosts(T)
    ref = host.loop(S(**sp_kw), TEMPLATE, 0, FIRST_AT_0, 0, N, drafts=[])[0]
    at = next(i for i in range(2, N) if ref[i] not in ref[:i] and i % T != T - 1)  # new to the stream, not a step's last token under perfect drafts
    sp = S(stop=[ref[at]], **sp_kw)
    s, m = spec_session(be, tiny(), T)
    c = create(be, TEMPLATE)
    for drafts in (ref, [], None):
        want = host.loop(sp, TEMPLATE, 0, FIRST_AT_0, 0, N, drafts=drafts, stop=[ref[at]])
        assert want[1] == at + 1 and want[0][:at + 1] == ref[:at + 1]
        state = 0
        for t in want[0][:at + 1]:
            state = TEMPLATE.advance(state, t)
        assert want[3] == state  # the state has advanced over the stop token too
        assert device(be, s, c, 0, FIRST_AT_0, 0, N, sp, drafts=drafts) == want
    s.set_constraint(None)
    s.close(), m.close()
    be.constraint_free(c)


# ── 5. two calls equal one ─────────────────────────────────────────────────────────────────────────────────────────────

def test_two_calls_equal_one_behind_prefill_and_sample(hip_backend, hosts):
    """resident_prefill fills the cache, zgml_hip_sample picks the first token over the last row and advances the device state, the
    constrained loop goes on from it in two calls: the state is carried by the device"""
    be, cfg, T, sp = hip_backend, tiny(), 4, S(**SP)
    p, host = prompt(cfg), hosts(T, PROMPT_LEN)
    host.s.prefill(p[PROMPT_LEN - T:], PROMPT_LEN - T, want_logits=False)
    first, state1 = c_constraint_sample(host.download()[T - 1], sp, PROMPT_LEN - 1, None, TEMPLATE, 0)
    assert first >= 0
    one = host.loop(sp, TEMPLATE, state1, first, PROMPT_LEN, N, history=p)
    a_want = host.loop(sp, TEMPLATE, state1, first, PROMPT_LEN, 10, history=p)
    b_want = host.loop(sp, TEMPLATE, a_want[3], a_want[0][9], PROMPT_LEN + 10, 14, history=p + [first] + a_want[0][:9])
    assert a_want[1] == 10 and b_want[1] == 14 and a_want[0] + b_want[0] == one[0] and b_want[3] == one[3]
    s, m = spec_session(be, cfg, T)
    c = create(be, TEMPLATE)
    s.set_constraint(c, 0)
    for chunk in range(PROMPT_LEN // T):
        s.resident_prefill(p[chunk * T:(chunk + 1) * T], chunk * T)
    tok, _ = be.sample(s.handle, m.buf("logits"), (T - 1) * V, V, sp, PROMPT_LEN - 1)
    assert tok == first and s.constraint_state() == state1
    a, na, sa = s.resident_decode_speculative_constrained(tok, PROMPT_LEN, 10, sp, history=p)
    assert (a.tolist(), na, sa, s.constraint_state()) == a_want
    b, nb, sb = s.resident_decode_speculative_constrained(int(a[9]), PROMPT_LEN + 10, 14, sp, history=p + [tok] + a[:9].tolist())
    assert (b.tolist(), nb, sb, s.constraint_state()) == b_want and not be.last_error(), be.last_error()
    assert a.tolist() + b.tolist() == one[0] and s.constraint_state() == one[3]
    s.set_constraint(None)
    s.close(), m.close()
    be.constraint_free(c)


# ── 6. against the other speculative entry points ──────────────────────────────────────────────────────────────────────

def test_against_the_other_speculative_entry_points(hip_backend):
    be, cfg, T = hip_backend, tiny(), 4
    everything = Dfa(np.zeros(V, u16), np.zeros((1, 1), u16))  # 1 state, 1 class, every token allowed
    s, m = spec_session(be, cfg, T)
    c = create(be, everything)
    for sp in (S(**SP), S(**SP, **PEN4), S(seed=3, **PARAMS["k1"])):
        stream = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, N + T - 1, sp, drafts=[])[0].tolist()
        for form in ALL_FORMS:
            drafts = drafts_for(form, stream, V)
            d0 = _dispatches(be, s.handle)
            toks, produced, stats = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, N, sp, drafts=drafts)
            d1 = _dispatches(be, s.handle)
            # no constraint attached: the sampled form, to the launch
            t2, p2, st2 = s.resident_decode_speculative_constrained(FIRST_AT_0, 0, N, sp, drafts=drafts)
            d2 = _dispatches(be, s.handle)
            assert (t2.tolist(), p2, st2) == (toks.tolist(), produced, stats) and (d2[0] - d1[0], d2[1] - d1[1]) == (d1[0] - d0[0], d1[1] - d0[1]), form
            # the all-allowing automaton: bit-equal tokens and statistics
            got = device(be, s, c, 0, FIRST_AT_0, 0, N, sp, drafts=drafts)
            assert got == (toks.tolist(), produced, stats, 0), form
            s.set_constraint(None)
            if sp.top_k == 1:  # constrained greedy speculation is the greedy form
                g_toks, g_stats = s.resident_decode_speculative(FIRST_AT_0, 0, N, drafts=drafts)
                assert (g_toks.tolist(), g_stats) == (got[0], got[2]), form
    assert not be.last_error(), be.last_error()
    s.close(), m.close()
    be.constraint_free(c)


# ── 7. alternation on one program ──────────────────────────────────────────────────────────────────────────────────────

def test_constrained_sampled_and_prefill_alternate_on_one_program(hip_backend, hosts):
    be, cfg, T, sp = hip_backend, tiny(), 4, S(**SP)
    want = hosts(T).loop(sp, TEMPLATE, 0, FIRST_AT_0, 0, N)
    s, m = spec_session(be, cfg, T)
    c = create(be, TEMPLATE)
    chunk = prompt(cfg, T)
    seen = []
    for _ in range(3):
        d0 = _dispatches(be, s.handle)
        con = device(be, s, c, 0, FIRST_AT_0, 0, N, sp)
        d1 = _dispatches(be, s.handle)
        s.set_constraint(None)
        plain = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, N, sp)
        d2 = _dispatches(be, s.handle)
        nxt = s.resident_prefill(chunk, 0)
        d3 = _dispatches(be, s.handle)
        seen.append((con, plain[0].tolist(), plain[1:], nxt, [(b[0] - a[0], b[1] - a[1]) for a, b in ((d0, d1), (d1, d2), (d2, d3))]))
    assert not be.last_error(), be.last_error()
    assert seen[0][0] == want and seen[0][1] != want[0]  # the constraint does something
    assert seen[1] == seen[0] and seen[2] == seen[0]  # results repeat, and every call launches what it launched before
    s.close(), m.close()
    be.constraint_free(c)


# ── 8. log-probabilities and alternatives ──────────────────────────────────────────────────────────────────────────────

def test_logprobs_and_alternatives_are_over_the_raw_rows_of_the_emitting_steps(hip_backend, hosts):
    be, T, a, sp = hip_backend, 4, 5, S(**SP, **PEN4)
    host = hosts(T)
    s, m = spec_session(be, tiny(), T)
    nan = 0x7FC00000
    # the template from state 0 (everything is produced) and a chain that ends after six tokens (NaN / -1 behind n_produced)
    for dfa, n_want in ((TEMPLATE, N), (chain_dfa(V, 7), 6)):
        c = create(be, dfa)
        want = host.loop(sp, dfa, 0, FIRST_AT_0, 0, N, values=a)
        assert want[1] == n_want
        rows = [host.rows[p] for p in range(n_want)]
        if dfa is TEMPLATE:  # precondition: the raw row's maximum is listed although the state forbids it
            assert sum(not dfa.allowed(r["state"])[r["top"][0][0]] for r in rows) > 0
        s.set_constraint(c, 0)
        toks, produced, stats, lps, (alt_tok, alt_val) = s.resident_decode_speculative_constrained(FIRST_AT_0, 0, N, sp, top_logprobs=a)
        assert not be.last_error(), be.last_error()
        assert (toks.tolist(), produced, stats, s.constraint_state()) == want
        assert lps.view(np.uint32)[:n_want].tolist() == [r["lp"] for r in rows]
        assert alt_tok[:n_want].tolist() == [r["top"][0] for r in rows] and alt_val.view(np.uint32)[:n_want].tolist() == [r["top"][1] for r in rows]
        assert np.all(lps.view(np.uint32)[n_want:] == nan) and np.all(alt_tok[n_want:] == -1) and np.all(alt_val.view(np.uint32)[n_want:] == nan)
        s.set_constraint(c, 0)
        t2, p2, _, lps2 = s.resident_decode_speculative_constrained(FIRST_AT_0, 0, N, sp, logprobs=True)
        assert t2.tolist() == want[0] and p2 == n_want and lps2.view(np.uint32).tolist() == lps.view(np.uint32).tolist()
        s.set_constraint(None)
        be.constraint_free(c)
    s.close(), m.close()


# ── 9. a multi-slice vocabulary ────────────────────────────────────────────────────────────────────────────────────────

def test_l7_dimensions_every_row_is_masked_with_its_own_state(hip_backend):
    """Two layers at Llama-2-7B dimensions, T = 4, 12 tokens: vocab 32000 is 18 slices per row. Consecutive states allow DISJOINT
    hashed classes, so a row masked with row 0's state instead of its own would pick a token its state forbids."""
    be, T, n, first = hip_backend, 4, 12, 20000
    cfg, sp = l7cfg(2), S(1.0, 40, 0.9, seed=31, stream=4)
    vocab = cfg.vocab_size
    nxt = np.full((4, 8), FORBIDDEN, u16)
    for st in range(4):
        nxt[st, 2 * st] = nxt[st, 2 * st + 1] = (st + 1) % 4
    dfa = Dfa(hashed_classes(vocab, 8), nxt)
    assert all(not np.any(dfa.allowed(a) & dfa.allowed(b)) for a in range(4) for b in range(a)) and all(dfa.allowed(a).sum() > 256 for a in range(4))
    host = Host(be, cfg, T, threads=16)
    s, m = spec_session(be, cfg, T, threads=16)
    c = create(be, dfa)
    stream = host.loop(sp, dfa, 0, first, 0, n + T - 1, drafts=[])[0]
    wrong = [(t + 8) % vocab if i in (2, 7) else t for i, t in enumerate(stream)]
    for drafts in (None, stream, wrong, []):
        want = host.loop(sp, dfa, 0, first, 0, n, drafts=drafts)
        assert want[1] == n and want[3] == n % 4
        if drafts is stream:
            assert want[2]["accepted"] == want[2]["drafted"] > 0  # rows behind row 0 are used
        got = device(be, s, c, 0, first, 0, n, sp, drafts=drafts)
        print(got[2])
        assert got == want
    s.set_constraint(None)
    for x in (s, m, host):
        x.close()
    be.constraint_free(c)


# ── 10. refusals ───────────────────────────────────────────────────────────────────────────────────────────────────────

def test_refusals_enqueue_nothing_and_the_next_call_works(hip_backend, hosts):
    be, cfg, T = hip_backend, tiny(), 4
    hip = capi.load_hip()
    good = S(**SP)
    s, m = spec_session(be, cfg, T)
    c = create(be, TEMPLATE)
    s.set_constraint(c, 0)
    m1 = llama.Model(cfg, llama.Q4_0)
    s1 = llama.Session(m1, llama.hip_backend_fns(be))
    s1.resident_setup(be)
    bm = llama.BatchModel(cfg, 2, llama.Q4_0, tokens_per_seq=2)
    sb = llama.BatchSession(bm, llama.hip_backend_fns(be), 2)
    sb.resident_setup(be)
    before = {x: _dispatches(be, x.handle) for x in (s, s1, sb)}

    def refused(call, text):
        with pytest.raises(RuntimeError, match=text):
            call()
        hip.zgml_hip_clear_error(be.ctx)
        for x in (s, s1, sb):
            assert _dispatches(be, x.handle) == before[x], text
        assert s.constraint_state() == 0

    for kw, text in BAD_PARAMS + [(dict(stop=[V]), "stop token"), (dict(recent=[1, 2], **PEN4), "recent must be NULL")]:
        refused(lambda: s.resident_decode_speculative_constrained(1, 0, 4, S(**kw)), text)
    refused(lambda: s.resident_decode_speculative_constrained(V, 0, 4, good), "token out of range")
    refused(lambda: s.resident_decode_speculative_constrained(1, 0, cfg.max_seq_len - T + 2, good), "max_seq")
    refused(lambda: s1.resident_decode_speculative_constrained(1, 0, 4, good), "token_len = 1")
    out, n_out = np.zeros(4, np.int64), C.c_uint32(7)
    assert hip.zgml_hip_resident_decode_speculative_constrained(be.ctx, sb.handle, 1, 0, 4, None, C.byref(good), out.ctypes.data, C.byref(n_out), None) == -1
    assert "batched" in be.last_error() and n_out.value == 0
    hip.zgml_hip_clear_error(be.ctx)
    assert hip.zgml_hip_resident_decode_speculative_constrained(be.ctx, s.handle, 1, 0, 4, None, None, out.ctypes.data, None, None) == -1
    assert "no sampling parameters" in be.last_error()
    hip.zgml_hip_clear_error(be.ctx)
    # the three existing speculative calls still refuse a program with a constraint attached
    sb.set_constraint(c, 0, seq=1)
    refused(lambda: s.resident_decode_speculative(FIRST_AT_0, 0, 8), "constraint is attached")
    refused(lambda: s.resident_decode_speculative_sampled(FIRST_AT_0, 0, 8, good), "constraint is attached")
    refused(lambda: sb.resident_decode_batch_speculative([1, 2], [0, 0], [3, 3]), "constraint is attached")
    sb.set_constraint(None, seq=1)
    # the next valid call gives what the reference gives
    assert device(be, s, c, 0, FIRST_AT_0, 0, N, good) == hosts(T).loop(good, TEMPLATE, 0, FIRST_AT_0, 0, N)
    s.set_constraint(None)
    for x in (s, m, s1, m1, sb, bm):
        x.close()
    be.constraint_free(c)
    assert not be.last_error(), be.last_error()
