"""Speculative decode with a draft model on the MI355X (zgml_hip_resident_decode_speculative_model): a token_len = T target plan
verifies what a second, token_len = 1 program drafts greedily, both resident, one graph launch per step.

Two references, as in tests/test_hip_spec_decode.py and tests/test_hip_spec_sampled.py:
  * from position 0 on the tiny model, the decode plan's resident stream (= the oracle's under THE TIE CONDITION that module
    asserts) for the tokens, and the oracle's statistics (tests/test_spec_draft_model_host.py, which also asserts that draft B's
    own picks are no near-ties);
  * everywhere else THE HOST-DRIVEN LOOP on the same backend: a second target T-plan through Session.prefill with all T rows
    downloaded, a second draft session through Session.step, fed to tests/spec_draft_model.py. Same kernels, same inputs:
    tokens and statistics identical, no tolerance. The sampled form samples the rows with tests/cpp/sample_probe.cpp (c_sample),
    the draft stays greedy.
Every condition a case depends on (a step that rejects, a step that accepts in part) is asserted on the reference alone."""
import ctypes as C

import numpy as np
import pytest

from zgml_amd import capi, llama
from tests.spec_draft_model import spec_draft_loop
from tests.test_hip_l7dims import l7cfg
from tests.test_hip_sample import PARAMS
from tests.test_hip_spec_decode import (FIRST_AT_0, FIRST_AT_8, FIRST_INT8, N, PROMPT_LEN, _dispatches, _download, decode_plan_stream, oracle_stream,
                                        prompt, spec_session, tiny)
from tests.test_logprob_host import c_logprob
from tests.test_penalty_host import c_sample_penalized
from tests.test_sample_host import c_sample
from tests.test_spec_draft_model_host import DRAFT_B
from tests.test_top_logprob_host import c_top

pytestmark = pytest.mark.gpu
S = capi.SamplingC.of
PEN4 = dict(repeat_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25, penalty_window=4)
SEED = 7  # of the sampled cases: chosen from the host-driven reference alone (a step with 0 < accepted < T - 1), then left fixed


def draft_b(kvq=0, max_seq=64):
    cfg = llama.preset("tiny", max_seq)
    cfg.n_layers, cfg.d_ff, cfg.kv_quant_block = 1, 128, kvq
    return cfg


def draft_session(be, cfg=None, like=None, small_m=None, threads=8, setup=True):
    """a token_len = 1 session with a resident set-up: over `cfg`, or over the weights of `like` (draft A on the target's own)"""
    m = llama.Model(cfg, llama.Q4_0, threads=threads, like=like)
    if small_m is not None:
        be.set_option(capi.OPT_SMALL_M_MATVEC, int(small_m))
    try:
        s = llama.Session(m, llama.hip_backend_fns(be))
    finally:
        if small_m is not None:
            be.set_option(capi.OPT_SMALL_M_MATVEC, 0)
    if setup:
        s.resident_setup(be)
    return s, m


def close(*xs):
    for x in xs:
        x.close()


class HostPair:
    """The reference side: a target T-plan and a draft of their own, driven from the host."""

    def __init__(self, be, tcfg, T, dcfg=None, like_target=False, small_m=None, threads=8):
        self.be, self.T, self.V = be, T, tcfg.vocab_size
        self.ts, self.tm = spec_session(be, tcfg, T, small_m=small_m, threads=threads)
        self.ds, self.dm = draft_session(be, dcfg, like=self.tm if like_target else None, small_m=small_m, threads=threads, setup=False)
        self.last_rows = None

    def fill(self, tokens):
        for pos, t in enumerate(tokens):
            self.ds.step(t, pos, want_logits=False)
        for at in range(0, len(tokens), self.T):
            self.ts.prefill(tokens[at:at + self.T], at, want_logits=False)

    def logits(self, c, pos):
        self.ts.prefill(c, pos, want_logits=False)
        self.last_rows = _download(self.be, self.ts.handle, self.tm.buf("logits"), self.T * self.V).reshape(self.T, self.V).copy()
        return self.last_rows

    def rows_greedy(self, c, pos):
        return [int(np.argmax(r)) for r in self.logits(c, pos)]

    def rows_sampled(self, sp, pen=None, known=None):
        """row j under sp at position pos + j; with penalties its window is the call's confirmed tokens and c[1..j]. `known`: a
        list the caller keeps — the tokens at positions lo .. pos (the loop's on_step extends it)"""
        def rows(c, pos):
            lg = self.logits(c, pos)
            if pen is None:
                return [c_sample(lg[j], sp, pos + j) for j in range(self.T)]
            return [c_sample_penalized(lg[j], sp, pos + j, known + [int(t) for t in c[1:j + 1]]) for j in range(self.T)]
        return rows

    def draft(self, tok, pos):
        return self.ds.step(tok, pos, want_logits=False)[0]

    def loop(self, first, start, n, rows=None, **kw):
        return spec_draft_loop(rows or self.rows_greedy, self.draft, first, start, n, self.T, **kw)

    def close(self):
        close(self.ds, self.dm, self.ts, self.tm)  # (the draft may be built over the target's weights)


def full(T, n=N):
    steps = -(-n // T)
    return {"steps": steps, "drafted": steps * (T - 1), "accepted": steps * (T - 1)}


def assert_draft_cache_is_in_step(be, d, fresh, confirmed):
    """The cache contract on the draft's side: after a call that confirmed `confirmed` (the tokens at positions 0 .. n), the draft's
    cache holds every column < n — the catch-up columns of the T-th executions among them. One vtable step of the draft at
    position n on confirmed[n] must give the logits of a fresh draft stepped over the whole confirmed sequence: the same plan on
    the same inputs, held to the parity bar of tests/test_hip_spec_decode.py, 2e-4 of the logit range (on the oracle a missing
    catch-up column moves these logits by 0.15 and more: tests/test_spec_draft_model_host.py)."""
    n = len(confirmed) - 1
    got = d.step(confirmed[n], n)[1]
    f, fm = fresh()
    for pos, t in enumerate(confirmed[:n]):
        f.step(t, pos, want_logits=False)
    want = f.step(confirmed[n], n)[1]
    close(f, fm)
    err = float(np.abs(got - want).max()) / float(np.abs(want).max())
    print("draft cache:", "bit-equal" if np.array_equal(got, want) else err)
    assert err <= 2e-4, err


# ── 1. greedy, drafts A and B, from position 0 ─────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("T", [2, 4, 5])
def test_tokens_and_stats_from_position_0(hip_backend, oracle, T):
    cfg = tiny()
    ref = oracle_stream(oracle, 0, FIRST_AT_0, 0)
    stream = decode_plan_stream(hip_backend, cfg, FIRST_AT_0, 0, N + T - 1)
    assert stream == ref[:N + T - 1]
    s, m = spec_session(hip_backend, cfg, T)
    # draft A over the target's own weights: accepted in full; its cache must have kept up — the column of every T-th execution
    da, dam = draft_session(hip_backend, like=m)
    toks, stats = s.resident_decode_speculative_model(da, FIRST_AT_0, 0, N)
    assert not hip_backend.last_error(), hip_backend.last_error()
    print(T, "A", stats)
    assert toks.tolist() == stream[:N] and stats == full(T)
    assert_draft_cache_is_in_step(hip_backend, da, lambda: draft_session(hip_backend, like=m, setup=False), [FIRST_AT_0] + stream[:N])
    db, dbm = draft_session(hip_backend, draft_b())
    toks, stats = s.resident_decode_speculative_model(db, FIRST_AT_0, 0, N)
    assert not hip_backend.last_error(), hip_backend.last_error()
    print(T, "B", stats)
    assert toks.tolist() == stream[:N]
    assert (stats["steps"], stats["drafted"], stats["accepted"]) == DRAFT_B[T]
    assert_draft_cache_is_in_step(hip_backend, db, lambda: draft_session(hip_backend, draft_b(), setup=False), [FIRST_AT_0] + stream[:N])
    close(da, dam, db, dbm, s, m)


# ── 2. behind a prompt ─────────────────────────────────────────────────────────────────────────────────────────────────

def test_behind_a_prompt_equals_the_host_driven_loop(hip_backend):
    """T = 4 from position 8 with a one-layer draft: resident_prefill chunks fill the target's cache, vtable steps the draft's"""
    cfg, T, p = tiny(), 4, prompt(tiny())
    host = HostPair(hip_backend, cfg, T, draft_b())
    host.fill(p)
    accepted = []
    want, produced, want_stats = host.loop(FIRST_AT_8, PROMPT_LEN, N, on_step=lambda pos, c, g, a, m: accepted.append(a))
    print(want_stats, accepted)
    assert produced == N and 0 in accepted and T - 1 in accepted  # condition: a step that rejects everything, one that accepts everything
    s, m = spec_session(hip_backend, cfg, T)
    d, dm = draft_session(hip_backend, draft_b(), setup=False)
    for chunk in range(PROMPT_LEN // T):
        s.resident_prefill(p[chunk * T:(chunk + 1) * T], chunk * T)
    for pos, t in enumerate(p):
        d.step(t, pos, want_logits=False)
    d.resident_setup(hip_backend)
    for history in (p, None):
        toks, stats = s.resident_decode_speculative_model(d, FIRST_AT_8, PROMPT_LEN, N, history=history)
        assert not hip_backend.last_error(), hip_backend.last_error()
        assert toks.tolist() == want and stats == want_stats, history
    close(host, s, m, d, dm)


# ── 3. two calls equal one ─────────────────────────────────────────────────────────────────────────────────────────────

def test_two_calls_equal_one_and_the_sessions_still_step(hip_backend):
    cfg, T = tiny(), 4
    host = HostPair(hip_backend, cfg, T, draft_b())
    w_a, _, st_a = host.loop(FIRST_AT_0, 0, 10)
    w_b, _, st_b = host.loop(w_a[-1], 10, 14)  # (the model's statistics from the state the first call left)
    s, m = spec_session(hip_backend, cfg, T)
    d, dm = draft_session(hip_backend, draft_b())
    one, st_one = s.resident_decode_speculative_model(d, FIRST_AT_0, 0, N)
    a, sa = s.resident_decode_speculative_model(d, FIRST_AT_0, 0, 10)
    b, sb = s.resident_decode_speculative_model(d, int(a[9]), 10, 14, history=[FIRST_AT_0] + a[:9].tolist())
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert a.tolist() + b.tolist() == one.tolist() == w_a + w_b
    assert sa == st_a and sb == st_b
    # both programs still step through the vtable, like fresh ones
    fs, fm = spec_session(hip_backend, cfg, T)
    fd, fdm = draft_session(hip_backend, draft_b(), setup=False)
    chunk = prompt(cfg, T)
    t_a, l_a = s.prefill(chunk, 0)
    t_b, l_b = fs.prefill(chunk, 0)
    assert t_a == t_b and np.array_equal(l_a, l_b)
    t_a, l_a = d.step(chunk[0], 0)
    t_b, l_b = fd.step(chunk[0], 0)
    assert t_a == t_b and np.array_equal(l_a, l_b) and not hip_backend.last_error()
    close(host, s, m, d, dm, fs, fm, fd, fdm)


# ── 4. the last step is cut ────────────────────────────────────────────────────────────────────────────────────────────

def test_the_last_step_is_cut_and_nothing_is_written_behind_the_tokens(hip_backend, oracle):
    """draft A, 9 tokens, T = 4: steps of 4, 4 and 1 — the last accepts three candidates and emits one"""
    cfg, T, n = tiny(), 4, 9
    stream = oracle_stream(oracle, 0, FIRST_AT_0, 0)
    s, m = spec_session(hip_backend, cfg, T)
    d, dm = draft_session(hip_backend, like=m)
    out = np.full(n + 8, -77, np.int64)
    stats, produced = capi.SpecStatsC(), C.c_uint32(77)
    rc = capi.load_hip().zgml_hip_resident_decode_speculative_model(hip_backend.ctx, s.handle, d.handle, FIRST_AT_0, 0, n, None, 0, None, out.ctypes.data,
                                                                    C.byref(produced), C.byref(stats))
    assert rc == 0 and not hip_backend.last_error(), hip_backend.last_error()
    assert out[:n].tolist() == stream[:n] and np.all(out[n:] == -77) and produced.value == n
    assert (stats.steps, stats.drafted, stats.accepted) == (3, 9, 9)
    # n_produced = NULL and stats = NULL are allowed
    out2 = np.full(n, -1, np.int64)
    assert capi.load_hip().zgml_hip_resident_decode_speculative_model(hip_backend.ctx, s.handle, d.handle, FIRST_AT_0, 0, n, None, 0, None, out2.ctypes.data, None, None) == 0
    assert out2.tolist() == stream[:n]
    close(d, dm, s, m)


# ── 5. int8 KV ─────────────────────────────────────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("kvq_t,kvq_d", [(32, 0), (0, 32), (32, 32)])
def test_int8_kv_equals_the_host_driven_loop(hip_backend, kvq_t, kvq_d):
    T = 4
    host = HostPair(hip_backend, tiny(kvq_t), T, draft_b(kvq_d))
    want, produced, want_stats = host.loop(FIRST_INT8, 0, N)
    assert produced == N
    s, m = spec_session(hip_backend, tiny(kvq_t), T)
    d, dm = draft_session(hip_backend, draft_b(kvq_d))
    toks, stats = s.resident_decode_speculative_model(d, FIRST_INT8, 0, N)
    assert not hip_backend.last_error(), hip_backend.last_error()
    print(kvq_t, kvq_d, stats)
    assert toks.tolist() == want and stats == want_stats
    close(host, s, m, d, dm)


# ── 6. the sampled verify step ─────────────────────────────────────────────────────────────────────────────────────────

@pytest.fixture(scope="module")
def sampled_pair(hip_backend):
    """T = 4, draft A: host pair and device pair, shared by the sampled cases (every call starts at position 0)"""
    cfg, T = tiny(), 4
    host = HostPair(hip_backend, cfg, T, like_target=True)
    s, m = spec_session(hip_backend, cfg, T)
    d, dm = draft_session(hip_backend, like=m)
    yield host, s, d
    close(host, d, dm, s, m)


def test_sampled_verify_equals_the_host_driven_loop(hip_backend, sampled_pair):
    host, s, d = sampled_pair
    T, sp = host.T, S(seed=SEED, stream=0, **PARAMS["k40_p95"])
    accepted = []
    want, produced, want_stats = host.loop(FIRST_AT_0, 0, N, rows=host.rows_sampled(sp), on_step=lambda pos, c, g, a, m: accepted.append(a))
    print(want_stats, accepted)
    assert produced == N and len(set(want)) > 3            # condition: it does sample
    assert any(0 < a < T - 1 for a in accepted), accepted  # condition: a step accepted in part
    toks, n, stats = s.resident_decode_speculative_model(d, FIRST_AT_0, 0, N, sampling=sp)
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert toks.tolist() == want and n == N and stats == want_stats
    # a stop token ends the call early: the first token of the stream that is new to it, from index 3 on
    at = next(i for i in range(3, N - 2) if want[i] not in want[:i])
    sp_stop = S(seed=SEED, stream=0, stop=[want[at]], **PARAMS["k40_p95"])
    w2, p2, st2 = host.loop(FIRST_AT_0, 0, N, rows=host.rows_sampled(sp_stop), stop=[want[at]])
    assert p2 == at + 1 and w2 == want[:at + 1]
    toks, n, stats = s.resident_decode_speculative_model(d, FIRST_AT_0, 0, N, sampling=sp_stop)
    assert n == p2 and toks[:n].tolist() == w2 and np.all(toks[n:] == -1) and stats == st2
    assert not hip_backend.last_error(), hip_backend.last_error()


def test_sampled_verify_with_penalties(hip_backend, sampled_pair):
    host, s, d = sampled_pair
    sp = S(seed=SEED, stream=1, **PARAMS["k256_p1"], **PEN4)
    known = [FIRST_AT_0]
    want, produced, want_stats = host.loop(FIRST_AT_0, 0, N, rows=host.rows_sampled(sp, PEN4, known), on_step=lambda pos, c, g, a, m: known.extend(g[:m]))
    plain, _, _ = host.loop(FIRST_AT_0, 0, N, rows=host.rows_sampled(S(seed=SEED, stream=1, **PARAMS["k256_p1"])))
    assert produced == N and want != plain  # condition: the penalties matter to the reference
    toks, n, stats = s.resident_decode_speculative_model(d, FIRST_AT_0, 0, N, sampling=sp)
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert toks.tolist() == want and n == N and stats == want_stats


def test_sampled_verify_values_and_alternatives(hip_backend, sampled_pair):
    host, s, d = sampled_pair
    sp, a_top = S(seed=SEED, stream=0, **PARAMS["k40_p95"]), 5
    emitted = []  # the logits row that emitted every token
    want, produced, want_stats = host.loop(FIRST_AT_0, 0, N, rows=host.rows_sampled(sp), on_step=lambda pos, c, g, a, m: emitted.extend(host.last_rows[:m]))
    assert produced == N and len(emitted) == N
    toks, n, stats, lp, (alt, val) = s.resident_decode_speculative_model(d, FIRST_AT_0, 0, N, sampling=sp, logprobs=True, top_logprobs=a_top)
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert toks.tolist() == want and n == N and stats == want_stats
    want_lp = np.array([c_logprob(emitted[i], want[i]) for i in range(N)], np.float32)
    assert np.array_equal(lp.view(np.uint32), want_lp.view(np.uint32))
    tops = [c_top(r, a_top) for r in emitted]
    assert np.array_equal(alt, np.array([t[0] for t in tops]))
    assert np.array_equal(val.view(np.uint32), np.array([t[1] for t in tops], np.float32).view(np.uint32))
    # logprobs alone: the same values
    toks2, _, _, lp2 = s.resident_decode_speculative_model(d, FIRST_AT_0, 0, N, sampling=sp, logprobs=True)
    assert toks2.tolist() == want and np.array_equal(lp2.view(np.uint32), lp.view(np.uint32))


def test_top_k_1_equals_the_greedy_form(hip_backend, sampled_pair):
    _, s, d = sampled_pair
    g_toks, g_stats = s.resident_decode_speculative_model(d, FIRST_AT_0, 0, N)
    toks, n, stats = s.resident_decode_speculative_model(d, FIRST_AT_0, 0, N, sampling=S(seed=99, stream=3, **PARAMS["k1"]))
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert toks.tolist() == g_toks.tolist() and n == N and stats == g_stats == full(4)


# ── 7. the pair's graphs ───────────────────────────────────────────────────────────────────────────────────────────────

def test_pair_graphs_follow_the_draft_and_leave_other_calls_alone(hip_backend):
    cfg, T = tiny(), 4
    s, m = spec_session(hip_backend, cfg, T)
    da, dam = draft_session(hip_backend, like=m)
    db, dbm = draft_session(hip_backend, draft_b())
    sp = S(seed=SEED, stream=0, **PARAMS["k40_p95"])

    def run(d):
        g = s.resident_decode_speculative_model(d, FIRST_AT_0, 0, N)
        k = s.resident_decode_speculative_model(d, FIRST_AT_0, 0, N, sampling=sp)
        assert not hip_backend.last_error(), hip_backend.last_error()
        return (g[0].tolist(), g[1], k[0].tolist(), k[1], k[2])

    first_a, first_b = run(da), run(db)
    assert first_a[1] == full(T) and first_b[1] != first_a[1]  # condition: the two drafts are told apart by their statistics
    assert run(da) == first_a
    ngram = s.resident_decode_speculative(FIRST_AT_0, 0, N)
    plain_b = db.resident_decode(FIRST_AT_0, 0, N).tolist()
    close(db, dbm)  # freed: a new draft B may land at the old address
    db, dbm = draft_session(hip_backend, draft_b())
    assert run(db) == first_b
    # interleaved with the other loops of either program: nothing is invalidated, every result equals its first run
    for _ in range(2):
        again = s.resident_decode_speculative(FIRST_AT_0, 0, N)
        assert again[0].tolist() == ngram[0].tolist() and again[1] == ngram[1]
        assert run(db) == first_b
        assert db.resident_decode(FIRST_AT_0, 0, N).tolist() == plain_b
        assert run(da) == first_a
    db.resident_setup(hip_backend)  # set up again: the pair re-captures
    assert run(db) == first_b
    assert not hip_backend.last_error(), hip_backend.last_error()
    close(da, dam, db, dbm, s, m)


# ── 8. refusals, profile ───────────────────────────────────────────────────────────────────────────────────────────────

def test_refusals_enqueue_nothing_and_leave_both_programs_usable(hip_backend):
    cfg, T = tiny(), 4
    hip, V, Smax = capi.load_hip(), cfg.vocab_size, 32
    s, m = spec_session(hip_backend, cfg, T)
    d, dm = draft_session(hip_backend, draft_b(max_seq=Smax))  # the smaller cache of the pair
    good = s.resident_decode_speculative_model(d, FIRST_AT_0, 0, 8)
    before = (_dispatches(hip_backend, s.handle), _dispatches(hip_backend, d.handle))

    def refused(call, text):
        with pytest.raises(RuntimeError, match=text):
            call()
        hip.zgml_hip_clear_error(hip_backend.ctx)
        assert (_dispatches(hip_backend, s.handle), _dispatches(hip_backend, d.handle)) == before, text

    # of the request and the target, as zgml_hip_resident_decode_speculative
    refused(lambda: s.resident_decode_speculative_model(d, V, 0, 4), "token out of range")
    refused(lambda: s.resident_decode_speculative_model(d, 1, 2, 4, history=[1, V]), "token out of range")
    refused(lambda: s.resident_decode_speculative_model(d, 1, 3, 4, history=[1, 2]), "n_history")
    refused(lambda: s.resident_decode_speculative_model(d, 1, cfg.max_seq_len - T - 2, 4), "max_seq")
    refused(lambda: d.resident_decode_speculative_model(s, 1, 0, 4), "token_len = 1")  # (the target must be a T >= 2 plan)
    # ... with sampling, as the sampled form
    refused(lambda: s.resident_decode_speculative_model(d, 1, 0, 4, sampling=S(temperature=0.0, top_k=4, top_p=1.0)), "temperature")
    refused(lambda: s.resident_decode_speculative_model(d, 1, 0, 4, sampling=S(recent=[], seed=1, **PARAMS["k40_p95"], **PEN4)), "recent must be NULL")
    # of the draft
    refused(lambda: s.resident_decode_speculative_model(None, 1, 0, 4), "no draft")
    refused(lambda: s.resident_decode_speculative_model(s, 1, 0, 4), "target program itself")
    s2, m2 = spec_session(hip_backend, cfg, 2)
    refused(lambda: s.resident_decode_speculative_model(s2, 1, 0, 4), "token_len = 1 plan")
    bare, bm = draft_session(hip_backend, draft_b(), setup=False)
    refused(lambda: s.resident_decode_speculative_model(bare, 1, 0, 4), "no resident set-up")
    bat_m = llama.BatchModel(cfg, 2)
    bat = llama.BatchSession(bat_m, llama.hip_backend_fns(hip_backend), 2)
    bat.resident_setup(hip_backend)
    refused(lambda: s.resident_decode_speculative_model(bat, 1, 0, 4), "batched")
    other = draft_b()
    other.vocab_size = V // 2
    ov, ovm = draft_session(hip_backend, other)
    refused(lambda: s.resident_decode_speculative_model(ov, 1, 0, 4), "vocabulary")
    sh, shm = draft_session(hip_backend, draft_b())
    pt = capi.ShardPointC(shm.program.n_ops, shm.buf("logits"), 0, 0, V)
    assert hip.zgml_hip_shard_attach(hip_backend.ctx, sh.handle, C.byref(pt), 1, shm.buf("logits"), V) == 0
    refused(lambda: s.resident_decode_speculative_model(sh, 1, 0, 4), "sharded")
    # the draft's max_seq: start + n + T - 1 = 33 > 32
    refused(lambda: s.resident_decode_speculative_model(d, 1, Smax - T - 2, 4), "draft's max_seq")
    # a constraint on either program
    class_of, nxt = np.zeros(V, np.uint16), np.zeros((1, 1), np.uint16)  # one state, every token allowed
    con = hip_backend.constraint_create(class_of, nxt)
    d.set_constraint(con)
    refused(lambda: s.resident_decode_speculative_model(d, 1, 0, 4), "constraint is attached to the draft")
    d.set_constraint(None)
    s.set_constraint(con)
    refused(lambda: s.resident_decode_speculative_model(d, 1, 0, 4), "constraint is attached")
    s.set_constraint(None)
    hip_backend.constraint_free(con)
    # no tokens wanted: 0, nothing touched
    toks, stats = s.resident_decode_speculative_model(d, 1, 0, 0)
    assert toks.size == 0 and stats == {"steps": 0, "drafted": 0, "accepted": 0}
    assert (_dispatches(hip_backend, s.handle), _dispatches(hip_backend, d.handle)) == before
    # the allowed edge of the smaller cache: start + n + T - 1 == 32
    toks, _ = s.resident_decode_speculative_model(d, 1, Smax - T - 3, 4)
    assert toks.size == 4 and not hip_backend.last_error(), hip_backend.last_error()
    # ... and both programs are usable: the first call again
    again = s.resident_decode_speculative_model(d, FIRST_AT_0, 0, 8)
    assert again[0].tolist() == good[0].tolist() and again[1] == good[1] and not hip_backend.last_error()
    close(s, m, d, dm, s2, m2, bare, bm, bat, bat_m, ov, ovm, sh, shm)


def test_each_program_counts_its_own_launches_and_the_ngram_step_counts_what_it_did(hip_backend):
    cfg, T = tiny(), 4
    s, m = spec_session(hip_backend, cfg, T)
    d, dm = draft_session(hip_backend, like=m)

    def delta(sess, call):
        """-> (launches, executions) the call added to the session's runtime profile, and its result"""
        b = _dispatches(hip_backend, sess.handle)
        out = call()
        a = _dispatches(hip_backend, sess.handle)
        return a[0] - b[0], a[1] - b[1], out

    # one resident_prefill is [prep] [plan] [argmax x 2]: plan + 3 launches, on either program
    plan_t = delta(s, lambda: s.resident_prefill(prompt(cfg, T), 0))[0] - 3
    plan_d = delta(d, lambda: d.resident_prefill([1], 0))[0] - 3
    # zgml_hip_resident_decode_speculative, as before this call existed: [draft] [prep] [plan] [stage 1] [accept] per step that ran
    launches, ran, (_, stats) = delta(s, lambda: s.resident_decode_speculative(FIRST_AT_0, 0, N))
    assert ran >= stats["steps"] > 0 and launches == ran * (plan_t + 4)
    # the pair: full acceptance, N / T steps and no idle one; the target's tail is [stage 1] [accept], the draft runs T times per step
    before_d = _dispatches(hip_backend, d.handle)
    launches, ran, (_, stats) = delta(s, lambda: s.resident_decode_speculative_model(d, FIRST_AT_0, 0, N))
    after_d = _dispatches(hip_backend, d.handle)
    assert stats == full(T) and ran == N // T and launches == ran * (plan_t + 3 + 1)
    assert (after_d[0] - before_d[0], after_d[1] - before_d[1]) == (ran * T * (plan_d + 3), ran * T)
    # ... under a sampled verify the target's tail is [select] [merge + pick] [accept]; idle steps count on both programs
    before_d = _dispatches(hip_backend, d.handle)
    launches, ran, _ = delta(s, lambda: s.resident_decode_speculative_model(d, FIRST_AT_0, 0, N, sampling=S(seed=SEED, **PARAMS["k40_p95"])))
    after_d = _dispatches(hip_backend, d.handle)
    assert launches == ran * (plan_t + 3 + 2) and after_d[0] - before_d[0] == ran * T * (plan_d + 3)
    # ... and the n-gram step afterwards counts what it counted
    again = delta(s, lambda: s.resident_decode_speculative(FIRST_AT_0, 0, N))
    assert again[0] == again[1] * (plan_t + 4) and not hip_backend.last_error()
    close(d, dm, s, m)


# ── 9. Llama-2-7B dimensions ───────────────────────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("small_m", [1, 0])
def test_l7_dimensions_device_loop_equals_the_host_driven_loop(hip_backend, small_m):
    """target: two layers at Llama-2-7B dimensions, T = 4; draft: one layer of the same dimensions; 12 tokens. The host-driven loop
    on the same plans is the only reference (tests/test_hip_spec_decode.py says why the tie condition cannot hold here)."""
    T, n, first = 4, 12, 20000
    host = HostPair(hip_backend, l7cfg(2), T, l7cfg(1), small_m=small_m, threads=16)
    want, produced, want_stats = host.loop(first, 0, n)
    assert produced == n
    s, m = spec_session(hip_backend, l7cfg(2), T, small_m=small_m, threads=16)
    assert ("qmatvec-kon-rows" in hip_backend.planText(s.handle)) == bool(small_m)
    d, dm = draft_session(hip_backend, l7cfg(1), small_m=small_m, threads=16)
    toks, stats = s.resident_decode_speculative_model(d, first, 0, n)
    assert not hip_backend.last_error(), hip_backend.last_error()
    print(small_m, stats)
    assert toks.tolist() == want and stats == want_stats
    close(host, s, m, d, dm)
