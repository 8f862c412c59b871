"""Speculative decode with a draft model under a constraint on the MI355X (zgml_hip_resident_decode_speculative_model_constrained):
the draft program's first maximum is taken over the tokens that the state of the TARGET's automaton allows, the walk gives every
verify row its state, and the verify step is the constrained one.

THE REFERENCE everywhere is THE HOST-DRIVEN LOOP on the same backend, fed to tests/spec_draft_constraint_model.py: a target T-plan of
its own through Session.prefill with all T rows downloaded and every row picked by zgml_amd/csrc/sample.h
(tests/cpp/constraint_probe.cpp: c_constraint_sample) under the state the model gave that row, and a draft of its own through
Session.step with its logits downloaded and the masked first maximum taken in numpy under the model's walk state. Same kernels,
same inputs: tokens, counts, statistics, states and log-probability bits are equal, no tolerance.

Every precondition — forced runs in the stream, a step that emits T tokens with a forced one among them, a step accepted in part,
a step in which the mask acts, a dead end where meant — is asserted on the reference alone, before the device loop is asked."""
import ctypes as C

import numpy as np
import pytest

from zgml_amd import capi
from tests import spec_constraint_model as SCM
from tests import spec_draft_constraint_model as SDM
from tests.test_constraint_host import Dfa, FORBIDDEN, c_constraint_sample
from tests.test_hip_constraint import hashed_classes, seeded_dfa
from tests.test_hip_l7dims import l7cfg
from tests.test_hip_penalty import PEN4
from tests.test_hip_sample import PARAMS
from tests.test_hip_spec_decode import FIRST_AT_0, FIRST_AT_8, FIRST_INT8, N, PROMPT_LEN, _dispatches, _download, prompt, spec_session, tiny
from tests.test_hip_spec_draft_model import assert_draft_cache_is_in_step, close, draft_b, draft_session
from tests.test_hip_spec_sampled import BAD_PARAMS
from tests.test_logprob_host import c_logprob
from tests.test_spec_constraint_host import chain_dfa, template_dfa
from tests.test_top_logprob_host import c_top

pytestmark = pytest.mark.gpu
S = capi.SamplingC.of
u16 = np.uint16
V = 512  # the tiny preset's vocabulary
SP = dict(seed=7, stream=0, **PARAMS["k40_p95"])  # the seed: chosen from the host-driven references alone (the preconditions of case 1), then left fixed
TEMPLATE, TEMPLATE_FREE, TEMPLATE_LITS = template_dfa(V, [0, 1, 0, 3, 0, 6], seed=21)  # literal runs of 1, 3 and 6 forced tokens between free states
SEEDED = seeded_dfa(11, V)
AUTOMATA = {"seeded": (SEEDED, 1), "template": (TEMPLATE, 0)}  # name -> (automaton, the state the walk starts in)


class HostPair:
    """The reference side: a target T-plan and a draft of their own, driven from the host; both caches hold the prompt below `start`."""

    def __init__(self, be, tcfg, T, dcfg=None, like_target=False, start=0, small_m=None, threads=8):
        self.be, self.T, self.V = be, T, tcfg.vocab_size
        self.ts, self.tm = spec_session(be, tcfg, T, small_m=small_m, threads=threads)
        self.ds, self.dm = draft_session(be, dcfg, like=self.tm if like_target else None, small_m=small_m, threads=threads, setup=False)
        p = prompt(tcfg, start)
        for pos, t in enumerate(p):
            self.ds.step(t, pos, want_logits=False)
        for at in range(0, start, T):
            self.ts.prefill(p[at:at + T], at, want_logits=False)
        self.last_rows = None

    def rows_fn(self, sp, dfa):
        def rows(c, pos, row_state, known):
            self.ts.prefill(c, pos, want_logits=False)
            self.last_rows = _download(self.be, self.ts.handle, self.tm.buf("logits"), self.T * self.V).reshape(self.T, self.V).copy()
            g = []
            for j in range(self.T):
                tok = -1 if row_state[j] == SCM.DEAD else c_constraint_sample(self.last_rows[j], sp, pos + j, known + c[1:j + 1], dfa, row_state[j])[0]
                g.append(tok if tok >= 0 else SCM.NO_PICK)
            return g
        return rows

    def draft(self, tok, pos):
        return self.ds.step(tok, pos)[1]

    def loop(self, sp, dfa, state, first, start, n, **kw):
        """-> (tokens, produced, statistics, the state afterwards)"""
        return SDM.spec_loop(self.rows_fn(sp, dfa), self.draft, first, start, n, self.T, dfa.class_of, dfa.next, state, **kw)

    def close(self):
        close(self.ds, self.dm, self.ts, self.tm)  # (the draft may be built over the target's weights)


class DevicePair:
    """The device side: a resident target T-plan and a resident draft (A: over the target's weights, B: one layer of its own)."""

    def __init__(self, be, tcfg, T, dcfg=None, like_target=False, small_m=None, threads=8):
        self.be = be
        self.s, self.m = spec_session(be, tcfg, T, small_m=small_m, threads=threads)
        self.d, self.dm = draft_session(be, dcfg, like=self.m if like_target else None, small_m=small_m, threads=threads)

    def run(self, c, state, first, start, n, sp, **kw):
        """one call from `state` -> (tokens, produced, statistics, the state afterwards)"""
        self.s.set_constraint(c, state)
        toks, produced, stats = self.s.resident_decode_speculative_model_constrained(self.d, first, start, n, sp, **kw)
        assert not self.be.last_error(), self.be.last_error()
        return toks.tolist(), produced, stats, self.s.constraint_state()

    def close(self):
        self.s.set_constraint(None)
        close(self.d, self.dm, self.s, self.m)


def pair_kw(draft):
    return dict(like_target=True) if draft == "A" else dict(dcfg=draft_b())


@pytest.fixture(scope="module")
def pairs(hip_backend):
    """host and device pairs of the tiny model, shared by the cases that start at position 0 (every call rewrites what it reads)"""
    made = {}

    def get(T, draft):
        if (T, draft) not in made:
            made[(T, draft)] = (HostPair(hip_backend, tiny(), T, **pair_kw(draft)), DevicePair(hip_backend, tiny(), T, **pair_kw(draft)))
        return made[(T, draft)]
    yield get
    for host, dev in made.values():
        host.close(), dev.close()


def create(be, dfa):
    return be.constraint_create(dfa.class_of, dfa.next)


def step_log(dfa, T):
    """-> (log, on_step): what every step of a reference loop did, for the preconditions"""
    frc = SCM.forced(dfa.class_of, dfa.next)
    log = []

    def on_step(pos, c, row_state, g, a, m, rows):
        log.append({"a": a, "m": m,
                    "forced_emitted": sum(frc[row_state[k]] != SCM.NO_FORCED for k in range(m)),
                    "mask_acts": any(row_state[j + 1] != SCM.DEAD and int(np.argmax(rows[j])) != c[j + 1] for j in range(T - 1))})
    return log, on_step


# ── 1. equals the host loop ────────────────────────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("pen", [{}, PEN4], ids=["plain", "penalties"])
@pytest.mark.parametrize("draft", ["A", "B"])
@pytest.mark.parametrize("which", ["seeded", "template"])
@pytest.mark.parametrize("T", [2, 4, 5])
def test_equals_the_host_loop(hip_backend, pairs, T, which, draft, pen):
    be = hip_backend
    host, dev = pairs(T, draft)
    dfa, state0 = AUTOMATA[which]
    sp = S(**SP, **pen)
    log, on_step = step_log(dfa, T)
    want = host.loop(sp, dfa, state0, FIRST_AT_0, 0, N, on_step=on_step)
    print(T, which, draft, want[2], [(x["a"], x["m"]) for x in log], sum(x["mask_acts"] for x in log), sum(x["forced_emitted"] for x in log))
    assert want[1] == N  # precondition: the walk goes on
    if which == "template":  # preconditions: forced runs in the stream; a step that emits T tokens, a forced one among them
        assert sum(x["forced_emitted"] for x in log) >= 8
        assert any(x["m"] == T and x["forced_emitted"] for x in log)
    else:  # precondition: in some step the masked draft is not the draft's plain first maximum
        assert any(x["mask_acts"] for x in log)
    if draft == "B":  # precondition: a step accepted in part (T = 2 has one draft per step: one step rejects it, one accepts it)
        acc = [x["a"] for x in log]
        assert any(0 < a < T - 1 for a in acc) if T > 2 else (0 in acc and 1 in acc), acc
    c = create(be, dfa)
    got = dev.run(c, state0, FIRST_AT_0, 0, N, sp)
    assert got == want
    dev.s.set_constraint(None)
    be.constraint_free(c)
    assert not be.last_error(), be.last_error()


# ── 2. a dead end ──────────────────────────────────────────────────────────────────────────────────────────────────────

def test_dead_end_finishes_the_call_in_front_of_the_empty_state(hip_backend, pairs):
    be, T, sp = hip_backend, 4, S(**SP)
    host, dev = pairs(T, "A")
    dfa = chain_dfa(V, 7)  # every token is allowed, six times; state 6 allows none
    log, on_step = step_log(dfa, T)
    want = host.loop(sp, dfa, 0, FIRST_AT_0, 0, N, on_step=on_step)
    print(want, log)
    # precondition: six tokens come out, the state stands in front of the empty state's row, the rest is -1
    assert want[1] == 6 and want[3] == 6 and want[0][6:] == [-1] * (N - 6) and -1 not in want[0][:6]
    c = create(be, dfa)
    assert dev.run(c, 0, FIRST_AT_0, 0, N, sp) == want
    # at row 0 of the first step: nothing is produced, one step, no draft (the state allows no token), no error on the context
    want0 = host.loop(sp, dfa, 6, FIRST_AT_0, 0, N)
    assert want0 == ([-1] * N, 0, {"steps": 1, "drafted": 0, "accepted": 0}, 6)
    assert dev.run(c, 6, FIRST_AT_0, 0, N, sp) == want0
    assert dev.run(c, 0, FIRST_AT_0, 0, N, sp) == want  # ... and the next call, from a live state, works
    dev.s.set_constraint(None)
    be.constraint_free(c)
    # both programs still step through the vtable, like fresh ones
    fs, fm = spec_session(be, tiny(), T)
    fd, fdm = draft_session(be, like=fm, setup=False)
    chunk = prompt(tiny(), T)
    t_a, l_a = dev.s.prefill(chunk, 0)
    t_b, l_b = fs.prefill(chunk, 0)
    assert t_a == t_b and np.array_equal(l_a, l_b)
    t_a, l_a = dev.d.step(chunk[0], 0)
    t_b, l_b = fd.step(chunk[0], 0)
    assert t_a == t_b and np.array_equal(l_a, l_b) and not be.last_error()
    close(fd, fdm, fs, fm)


# ── 3. two calls equal one, behind a prompt ────────────────────────────────────────────────────────────────────────────

def test_two_calls_equal_one_behind_a_prompt_and_the_drafts_cache_is_in_step(hip_backend):
    be, cfg, T, sp = hip_backend, tiny(), 4, S(**SP)
    p = prompt(cfg)
    host = HostPair(be, cfg, T, draft_b(), start=PROMPT_LEN)
    one = host.loop(sp, TEMPLATE, 0, FIRST_AT_8, PROMPT_LEN, N)
    a_want = host.loop(sp, TEMPLATE, 0, FIRST_AT_8, PROMPT_LEN, 10)
    b_want = host.loop(sp, TEMPLATE, a_want[3], a_want[0][9], PROMPT_LEN + 10, 14)
    assert one[1] == N and a_want[0] + b_want[0] == one[0] and b_want[3] == one[3]  # (the model's statistics from the state the first call left)
    dev = DevicePair(be, cfg, T, draft_b())
    for chunk in range(PROMPT_LEN // T):
        dev.s.resident_prefill(p[chunk * T:(chunk + 1) * T], chunk * T)
    for pos, t in enumerate(p):
        dev.d.step(t, pos, want_logits=False)
    c = create(be, TEMPLATE)
    for with_history in (True, False):  # (no penalties: the history is the window's business alone)
        assert dev.run(c, 0, FIRST_AT_8, PROMPT_LEN, N, sp, history=p if with_history else None) == one
        a = dev.run(c, 0, FIRST_AT_8, PROMPT_LEN, 10, sp, history=p if with_history else None)
        assert a == a_want
        hist_b = p + [FIRST_AT_8] + a[0][:9] if with_history else None
        toks, produced, stats = dev.s.resident_decode_speculative_model_constrained(dev.d, a[0][9], PROMPT_LEN + 10, 14, sp, history=hist_b)
        assert (toks.tolist(), produced, stats, dev.s.constraint_state()) == b_want and not be.last_error(), be.last_error()
    assert_draft_cache_is_in_step(be, dev.d, lambda: draft_session(be, draft_b(), setup=False), p + [FIRST_AT_8] + one[0])
    dev.s.set_constraint(None)
    be.constraint_free(c)
    close(host, dev)


# ── 4. large state rows ────────────────────────────────────────────────────────────────────────────────────────────────

def wide_dfa(n_states=4, n_classes=8192, seed=5):
    """8192 classes — a state row of 16 KiB —, the tokens in every 16th of them, all the others empty"""
    rng = np.random.default_rng(seed)
    nxt = rng.integers(0, n_states, (n_states, n_classes)).astype(u16)
    nxt[rng.random((n_states, n_classes)) < 0.5] = FORBIDDEN
    return Dfa((np.arange(V) * 16).astype(u16), nxt)


@pytest.mark.parametrize("which", ["one_class", "8192_classes"])
def test_large_and_small_state_rows(hip_backend, pairs, which):
    be, T, sp = hip_backend, 4, S(**SP)
    host, dev = pairs(T, "B")
    dfa = Dfa(np.zeros(V, u16), np.zeros((1, 1), u16)) if which == "one_class" else wide_dfa()
    if which == "8192_classes":  # precondition: empty classes, and every state forbids and allows many tokens
        assert dfa.n_classes == 8192 and np.unique(dfa.class_of).size == V and all(100 < dfa.allowed(s).sum() < V - 100 for s in range(dfa.n_states))
    log, on_step = step_log(dfa, T)
    want = host.loop(sp, dfa, 0, FIRST_AT_0, 0, N, on_step=on_step)
    assert want[1] == N and (which == "one_class" or any(x["mask_acts"] for x in log))
    c = create(be, dfa)
    assert dev.run(c, 0, FIRST_AT_0, 0, N, sp) == want
    dev.s.set_constraint(None)
    be.constraint_free(c)


def test_l7_dimensions_the_draft_is_masked_with_the_walks_state(hip_backend):
    """target: two layers at Llama-2-7B dimensions, T = 4; draft: one layer of the same dimensions; 12 tokens; vocabulary 32000 —
    32 workgroups per masked stage 1 — and a 16 KiB state row: 8192 hashed classes of about four tokens. Every state allows two
    classes, and consecutive states allow DISJOINT ones, so a draft masked with another row's state would be forbidden where it
    stands; among so few tokens the one-layer draft now and then agrees with the target, so rows behind row 0 emit."""
    be, T, n, first = hip_backend, 4, 12, 20000
    sp = S(1.0, 40, 0.9, seed=31, stream=4)
    vocab = l7cfg(2).vocab_size
    nxt = np.full((4, 8192), FORBIDDEN, u16)
    for st in range(4):
        nxt[st, 2 * st] = nxt[st, 2 * st + 1] = (st + 1) % 4
    dfa = Dfa(hashed_classes(vocab, 8192), nxt)
    assert all(not np.any(dfa.allowed(a) & dfa.allowed(b)) for a in range(4) for b in range(a)) and all(dfa.allowed(a).sum() >= 6 for a in range(4))
    host = HostPair(be, l7cfg(2), T, l7cfg(1), small_m=1, threads=16)
    log, on_step = step_log(dfa, T)
    want = host.loop(sp, dfa, 0, first, 0, n, on_step=on_step)
    print(want[2], [(x["a"], x["m"]) for x in log])
    assert want[1] == n and want[3] == n % 4 and any(x["mask_acts"] for x in log)
    assert want[2]["accepted"] > 0  # precondition: a row behind row 0 emits
    assert want[2]["drafted"] == want[2]["steps"] * (T - 1)  # every state allows tokens: every row is live
    dev = DevicePair(be, l7cfg(2), T, l7cfg(1), small_m=1, threads=16)
    assert "qmatvec-kon-rows" in be.planText(dev.s.handle)
    c = create(be, dfa)
    assert dev.run(c, 0, first, 0, n, sp) == want
    dev.s.set_constraint(None)
    be.constraint_free(c)
    close(host, dev)


# ── 5. int8 KV ─────────────────────────────────────────────────────────────────────────────────────────────────────────

def test_int8_kv_on_both_programs(hip_backend):
    be, T, sp = hip_backend, 4, S(**SP)
    host = HostPair(be, tiny(32), T, draft_b(32))
    want = host.loop(sp, SEEDED, 1, FIRST_INT8, 0, N)
    assert want[1] == N
    dev = DevicePair(be, tiny(32), T, draft_b(32))
    c = create(be, SEEDED)
    assert dev.run(c, 1, FIRST_INT8, 0, N, sp) == want
    dev.s.set_constraint(None)
    be.constraint_free(c)
    close(host, dev)


# ── 6. log-probabilities and alternatives ──────────────────────────────────────────────────────────────────────────────

def test_logprobs_and_alternatives_are_over_the_raw_rows_of_the_emitting_steps(hip_backend, pairs):
    be, T, a_top, sp = hip_backend, 4, 5, S(**SP, **PEN4)
    host, dev = pairs(T, "A")
    emitted = []  # the raw logits row that emitted every token
    want = host.loop(sp, TEMPLATE, 0, FIRST_AT_0, 0, N, on_step=lambda pos, c, rs, g, a, m, rows: emitted.extend(host.last_rows[:m]))
    assert want[1] == N and len(emitted) == N
    c = create(be, TEMPLATE)
    dev.s.set_constraint(c, 0)
    toks, produced, stats, lp, (alt, val) = dev.s.resident_decode_speculative_model_constrained(dev.d, FIRST_AT_0, 0, N, sp, logprobs=True, top_logprobs=a_top)
    assert not be.last_error(), be.last_error()
    assert (toks.tolist(), produced, stats, dev.s.constraint_state()) == want
    want_lp = np.array([c_logprob(emitted[i], want[0][i]) for i in range(N)], np.float32)
    assert np.array_equal(lp.view(np.uint32), want_lp.view(np.uint32))
    tops = [c_top(r, a_top) for r in emitted]
    assert np.array_equal(alt, np.array([t[0] for t in tops]))
    assert np.array_equal(val.view(np.uint32), np.array([t[1] for t in tops], np.float32).view(np.uint32))
    dev.s.set_constraint(c, 0)  # logprobs alone: the same values
    toks2, _, _, lp2 = dev.s.resident_decode_speculative_model_constrained(dev.d, FIRST_AT_0, 0, N, sp, logprobs=True)
    assert toks2.tolist() == want[0] and np.array_equal(lp2.view(np.uint32), lp.view(np.uint32))
    dev.s.set_constraint(None)
    be.constraint_free(c)


# ── 7. no constraint attached ──────────────────────────────────────────────────────────────────────────────────────────

def test_without_a_constraint_it_is_the_draft_model_call_to_the_launch(hip_backend, pairs):
    be, T = hip_backend, 4
    _, dev = pairs(T, "B")
    s, d = dev.s, dev.d
    s.set_constraint(None)

    def both():
        return _dispatches(be, s.handle), _dispatches(be, d.handle)

    def delta(a, b):
        return [(y[0] - x[0], y[1] - x[1]) for x, y in zip(a, b)]

    for sp in (S(**SP), S(**SP, **PEN4), S(seed=3, **PARAMS["k1"])):
        d0 = both()
        toks, produced, stats = s.resident_decode_speculative_model(d, FIRST_AT_0, 0, N, sampling=sp)
        d1 = both()
        t2, p2, st2 = s.resident_decode_speculative_model_constrained(d, FIRST_AT_0, 0, N, sp)
        d2 = both()
        assert (t2.tolist(), p2, st2) == (toks.tolist(), produced, stats) and delta(d1, d2) == delta(d0, d1)
    assert not be.last_error(), be.last_error()


# ── 8. graphs ──────────────────────────────────────────────────────────────────────────────────────────────────────────

def test_graphs_belong_to_the_pair_and_nothing_else_is_invalidated(hip_backend):
    be, cfg, T, sp = hip_backend, tiny(), 4, S(**SP)
    dev = DevicePair(be, cfg, T, draft_b())
    s = dev.s
    c_seeded, c_template = create(be, SEEDED), create(be, TEMPLATE)
    assert SEEDED.n_classes != TEMPLATE.n_classes  # (an automaton of another class count between calls)

    def under(c, state):
        return dev.run(c, state, FIRST_AT_0, 0, N, sp)

    def others():
        """the other loops of either program, under the same constraint where they honour one"""
        s.set_constraint(c_seeded, 1)
        con = s.resident_decode_speculative_constrained(FIRST_AT_0, 0, N, sp)
        s.set_constraint(None)
        model = s.resident_decode_speculative_model(dev.d, FIRST_AT_0, 0, N, sampling=sp)
        dev.d.set_constraint(c_seeded, 1)
        sampled = dev.d.resident_decode_sampled(FIRST_AT_0, 0, N, sp)
        dev.d.set_constraint(None)
        assert not be.last_error(), be.last_error()
        return [(x[0].tolist(),) + tuple(x[1:]) for x in (con, model, sampled)]

    first_seeded, first_template, first_others = under(c_seeded, 1), under(c_template, 0), others()
    assert first_seeded != first_template and first_seeded[0] != first_others[1][0]  # condition: the automata and the mask do something
    for _ in range(2):
        assert under(c_seeded, 1) == first_seeded
        assert others() == first_others
        assert under(c_template, 0) == first_template
    s.set_constraint(None)
    close(dev.d, dev.dm)  # freed: a new draft B may land at the old address
    dev.d, dev.dm = draft_session(be, draft_b())
    assert under(c_seeded, 1) == first_seeded and others() == first_others
    dev.d.resident_setup(be)  # set up again: the pair re-captures
    assert under(c_template, 0) == first_template
    s.set_constraint(None)
    be.constraint_free(c_seeded), be.constraint_free(c_template)
    assert not be.last_error(), be.last_error()
    dev.close()


# ── 9. launch counts ───────────────────────────────────────────────────────────────────────────────────────────────────

def test_each_program_counts_its_own_launches(hip_backend, pairs):
    be, T, sp = hip_backend, 4, S(**SP)
    _, dev = pairs(T, "A")
    s, d = dev.s, dev.d
    s.set_constraint(None)

    def delta(sess, call):
        b = _dispatches(be, sess.handle)
        out = call()
        a = _dispatches(be, sess.handle)
        return a[0] - b[0], a[1] - b[1], out

    # one resident_prefill is [prep] [plan] [argmax x 2]: plan + 3 launches, on either program
    plan_t = delta(s, lambda: s.resident_prefill(prompt(tiny(), T), 0))[0] - 3
    plan_d = delta(d, lambda: d.resident_prefill([1], 0))[0] - 3
    c = create(be, TEMPLATE)
    before_d = _dispatches(be, d.handle)
    launches, ran, got = delta(s, lambda: dev.run(c, 0, FIRST_AT_0, 0, N, sp))
    after_d = _dispatches(be, d.handle)
    # the target: [draft launch] [prep] [plan] [constrained-rows select] [merge + pick] [accept]; the draft: T x { [prep] [plan] [masked stage 1] [stage 2] }
    assert ran >= got[2]["steps"] > 0 and launches == ran * (plan_t + 3 + 2)
    assert (after_d[0] - before_d[0], after_d[1] - before_d[1]) == (ran * T * (plan_d + 3), ran * T)
    s.set_constraint(None)
    be.constraint_free(c)


# ── 10. refusals ───────────────────────────────────────────────────────────────────────────────────────────────────────

def test_refusals_enqueue_nothing_and_leave_both_programs_usable(hip_backend):
    be, cfg, T = hip_backend, tiny(), 4
    hip, Smax, good = capi.load_hip(), 32, S(**SP)
    dev = DevicePair(be, cfg, T, draft_b(max_seq=Smax))  # the smaller cache of the pair
    s, d = dev.s, dev.d
    c = create(be, TEMPLATE)
    first = dev.run(c, 0, FIRST_AT_0, 0, 8, good)
    s.set_constraint(c, 0)
    before = (_dispatches(be, s.handle), _dispatches(be, d.handle))
    call = s.resident_decode_speculative_model_constrained

    def refused(fn, text):
        with pytest.raises(RuntimeError, match=text):
            fn()
        hip.zgml_hip_clear_error(be.ctx)
        assert (_dispatches(be, s.handle), _dispatches(be, d.handle)) == before, text
        assert s.constraint_state() == 0

    # sampling == NULL
    out, n_out = np.zeros(4, np.int64), C.c_uint32(7)
    assert hip.zgml_hip_resident_decode_speculative_model_constrained(be.ctx, s.handle, d.handle, 1, 0, 4, None, 0, None, out.ctypes.data, C.byref(n_out), None) == -1
    assert "sampling is NULL" in be.last_error() and n_out.value == 0
    hip.zgml_hip_clear_error(be.ctx)
    with pytest.raises(ValueError):
        call(d, 1, 0, 4, None)
    # of the parameter set, as the sampled form
    for kw, text in BAD_PARAMS + [(dict(stop=[V]), "stop token"), (dict(recent=[1, 2], **PEN4), "recent must be NULL")]:
        refused(lambda: call(d, 1, 0, 4, S(**kw)), text)
    # of the request and the target
    refused(lambda: call(d, V, 0, 4, good), "token out of range")
    refused(lambda: call(d, 1, 2, 4, good, history=[1, V]), "token out of range")
    refused(lambda: call(d, 1, 3, 4, good, history=[1, 2]), "n_history")
    refused(lambda: call(d, 1, cfg.max_seq_len - T - 2, 4, good), "max_seq")
    refused(lambda: d.resident_decode_speculative_model_constrained(s, 1, 0, 4, good), "token_len = 1")  # (the target must be a T >= 2 plan)
    # of the draft
    refused(lambda: call(None, 1, 0, 4, good), "no draft")
    refused(lambda: call(s, 1, 0, 4, good), "target program itself")
    bare, bm = draft_session(be, draft_b(), setup=False)
    refused(lambda: call(bare, 1, 0, 4, good), "no resident set-up")
    other = draft_b()
    other.vocab_size = V // 2
    ov, ovm = draft_session(be, other)
    refused(lambda: call(ov, 1, 0, 4, good), "vocabulary")
    refused(lambda: call(d, 1, Smax - T - 2, 4, good), "draft's max_seq")  # start + n + T - 1 = 33 > 32
    d.set_constraint(c, 0)
    refused(lambda: call(d, 1, 0, 4, good), "constraint is attached to the draft")
    d.set_constraint(None)
    # the sibling keeps refusing the target's constraint, in the words it had
    refused(lambda: s.resident_decode_speculative_model(d, 1, 0, 4, sampling=good), "constraint is attached to the program")
    # no tokens wanted: 0, nothing touched
    toks, produced, stats = call(d, 1, 0, 0, good)
    assert toks.size == 0 and produced == 0 and stats == {"steps": 0, "drafted": 0, "accepted": 0}
    assert (_dispatches(be, s.handle), _dispatches(be, d.handle)) == before and s.constraint_state() == 0
    # both programs are usable: the first call again
    assert dev.run(c, 0, FIRST_AT_0, 0, 8, good) == first
    s.set_constraint(None)
    be.constraint_free(c)
    close(bare, bm, ov, ovm)
    dev.close()
    assert not be.last_error(), be.last_error()
