"""Speculative decode with a draft model under batching on the MI355X (zgml_hip_resident_decode_batch_speculative_model): every
sequence of a batched tokens_per_seq = T target plan verifies what a second, batched one-column program drafts greedily for it,
both resident, one graph launch per step.

References, as in tests/test_hip_spec_draft_model.py:
  * from position 0 on the tiny model, the decode plan's resident stream (= the oracle's under THE TIE CONDITION that
    tests/test_hip_spec_decode.py asserts) for the tokens, and the oracle's statistics
    (tests/test_batch_spec_draft_model_host.py, which also asserts that draft B's own picks are no near-ties);
  * everywhere else THE HOST-DRIVEN PAIR on the same backend: a second batched target session and a second batched draft session
    over the same weights, driven with BatchSession.step, all B T rows read, through tests/batch_spec_draft_model.py. Same plans,
    same inputs, same step grouping: tokens and statistics identical, no tolerance. The sampled cases pick with
    tests/cpp/sample_probe.cpp / penalty_probe.cpp (c_sample, c_sample_penalized); the drafts stay greedy.
Every condition a case depends on (a step that rejects, one that accepts in part, a stop inside a step) is asserted on the
reference alone."""
import ctypes as C

import numpy as np
import pytest

from zgml_amd import Backend, capi, llama
from tests import batch_spec_draft_model as BDM
from tests import test_hip_spec_decode as SD
from tests.test_hip_batch_spec_decode import admit_prompt, batch_session, stream_of
from tests.test_hip_l7dims import l7cfg
from tests.test_hip_sample import PARAMS
from tests.test_hip_spec_draft_model import PEN4, draft_b, draft_session
from tests.test_spec_draft_model_host import DRAFT_B

pytestmark = pytest.mark.gpu

S = capi.SamplingC.of
N, PROMPT_LEN = SD.N, SD.PROMPT_LEN
FIRST_AT_0, FIRST_AT_8, FIRST_INT8 = SD.FIRST_AT_0, SD.FIRST_AT_8, SD.FIRST_INT8
ZERO = {"steps": 0, "drafted": 0, "accepted": 0}
NAN_WORD = 0x7FC00000
FIRSTS, STARTS, COUNTS = [FIRST_AT_0, FIRST_AT_8, FIRST_AT_0], [0, PROMPT_LEN, 0], [N, 17, N]
_dispatches = SD._dispatches


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def full(T, n):
    steps = -(-n // T)
    return {"steps": steps, "drafted": steps * (T - 1), "accepted": steps * (T - 1)}


def admit_prompt_one_column(be, s, bm, seq):
    """admit_prompt for a one-column plan: the prompt stepped through a decode plan of the same weights, handed to sequence `seq`"""
    mp = llama.Model(bm.cfg, like=bm)
    sp = llama.Session(mp, llama.hip_backend_fns(be))
    p = SD.prompt(bm.cfg)
    for pos, t in enumerate(p):
        sp.step(t, pos, want_logits=False)
    s.admit(seq, sp, PROMPT_LEN)
    be.synchronize()
    sp.close(), mp.close()
    return p


def draft_batch_session(be, B, cfg=None, like=None, kvq=0, behind=(), threads=8, setup=True):
    """a batched one-column session — over `cfg`, or over the weights of `like` (draft A on the target's own) — with the prompt
    admitted to the sequences `behind` and, unless told otherwise, a resident set-up"""
    bm = llama.BatchModel(cfg, B, llama.Q4_0, threads=threads, like=like, kv_quant_block=kvq)
    s = llama.BatchSession(bm, llama.hip_backend_fns(be), B)
    for seq in behind:
        admit_prompt_one_column(be, s, bm, seq)
    if setup:
        s.resident_setup(be)
    return s, bm


class Pair:
    """The device side — target session `s` and draft session `d`, both resident — and the host-driven side, `hs` and `hd`, second
    sessions over the same two models; the sequences `behind` of all four sit behind the admitted prompt. dcfg=None: draft A, over
    the target's own weights."""

    def __init__(self, be, tcfg, B, T, dcfg=None, kvq_t=0, kvq_d=0, behind=(1,), threads=8):
        self.be, self.B, self.T, self.behind = be, B, T, behind
        self.s, self.tm = batch_session(be, tcfg, B, T, kvq=kvq_t, threads=threads)
        self.hs = llama.BatchSession(self.tm, llama.hip_backend_fns(be), B)
        self.prompt = None
        for seq in behind:
            self.prompt = admit_prompt(be, self.s, self.tm, seq, T)
            admit_prompt(be, self.hs, self.tm, seq, T)
        self.d, self.dm = draft_batch_session(be, B, dcfg, like=self.tm if dcfg is None else None, kvq=kvq_d, behind=behind, threads=threads)
        self.hd = llama.BatchSession(self.dm, llama.hip_backend_fns(be), B)
        for seq in behind:
            admit_prompt_one_column(be, self.hd, self.dm, seq)

    def want(self, rqs, **kw):
        return BDM.lockstep(lambda t, p: self.hs.step(t, p)[1], lambda t, p: self.hd.step(t, p)[1], self.T, rqs, **kw)

    def got(self, rqs, logprobs=None):
        sampled = rqs[0].sampling is not None
        out = self.s.resident_decode_batch_speculative_model(self.d, [r.first for r in rqs], [r.start for r in rqs], [r.n for r in rqs],
                                                             samplings=[r.sampling for r in rqs] if sampled else None,
                                                             histories=[r.history for r in rqs], logprobs=logprobs)
        assert not self.be.last_error(), self.be.last_error()
        return out

    def check(self, rqs, logprobs=None, tag="", **kw):
        """the device call equals the host-driven pair on the same requests -> the reference"""
        want = self.want(rqs, **kw)
        got = self.got(rqs, logprobs)
        print(tag, "produced", want[1], "stats", got[2])
        assert got[0].tolist() == want[0].tolist(), tag
        assert np.asarray(got[1]).tolist() == want[1] and got[2] == want[2], (tag, got[1], want[1], got[2], want[2])
        if logprobs is not None:
            for b in range(self.B):
                row = bits(want[3][b]) if logprobs[b] else np.full(want[3].shape[1], NAN_WORD, np.uint32)
                assert bits(got[3][b]).tolist() == row.tolist(), (tag, b)
        return want

    def fresh_draft(self):
        return draft_batch_session(self.be, self.B, like=self.dm, kvq=self.dm.kv_quant_block, behind=self.behind, setup=False)

    def close(self):
        for x in (self.hd, self.d, self.dm, self.hs, self.s, self.tm):  # (the draft may be built over the target's weights)
            x.close()


def three(pair, counts=COUNTS, samplings=(None, None, None)):
    return [BDM.Request(FIRSTS[b], STARTS[b], counts[b], samplings[b], history=[None, pair.prompt, None][b]) for b in range(3)]


def assert_draft_caches_are_in_step(pair, confirmed, starts):
    """tests/test_hip_spec_draft_model.assert_draft_cache_is_in_step for every sequence at once, through BatchSession.step:
    confirmed[b] are the tokens at positions starts[b] .. n_b. One step of the draft session on every sequence's last confirmed
    token must give the logits of a fresh draft session (the prompt admitted where the pair's is) stepped over the confirmed
    tokens — a sequence with fewer of them repeats its last column meanwhile, with the same values. The same plan on the same
    inputs, held to that check's bar: 2e-4 of the logit range."""
    B = pair.B
    last = [len(c) - 1 for c in confirmed]
    got = pair.d.step([confirmed[b][last[b]] for b in range(B)], [starts[b] + last[b] for b in range(B)])[1]
    f, fm = pair.fresh_draft()
    for i in range(max(last)):
        at = [min(i, max(last[b] - 1, 0)) for b in range(B)]
        f.step([confirmed[b][at[b]] for b in range(B)], [starts[b] + at[b] for b in range(B)])
    want = f.step([confirmed[b][last[b]] for b in range(B)], [starts[b] + last[b] for b in range(B)])[1]
    f.close(), fm.close()
    for b in range(B):
        err = float(np.abs(got[b] - want[b]).max()) / float(np.abs(want[b]).max())
        print("draft cache, sequence", b, "bit-equal" if np.array_equal(got[b], want[b]) else err)
        assert err <= 2e-4, (b, err)


# ── 1, 2. greedy, drafts A and B, from position 0 and behind a prompt; the draft's cache ───────────────────────────────────

@pytest.mark.parametrize("T", [2, 4, 5])
def test_tokens_and_stats_of_three_sequences(hip_backend, oracle, T):
    """B = 3: sequences 0 and 2 the same request from position 0, sequence 1 behind the prompt admitted into both sessions"""
    be = hip_backend
    streams = [stream_of(be, oracle, 0, f, st) for f, st in zip(FIRSTS, STARTS)]
    # draft A over the target's own weights: accepted in full by every sequence
    pair = Pair(be, SD.tiny(), 3, T)
    want = pair.check(three(pair), tag=f"T {T} A")
    for b in range(3):
        assert want[0][b, :COUNTS[b]].tolist() == streams[b][:COUNTS[b]] and np.all(want[0][b, COUNTS[b]:] == -1)
        assert want[2][b] == full(T, COUNTS[b]), b
    assert_draft_caches_are_in_step(pair, [[FIRSTS[b]] + streams[b][:COUNTS[b]] for b in range(3)], STARTS)
    pair.close()
    # draft B: the oracle's statistics for the sequences from position 0, the host-driven pair's for the one behind the prompt
    pair = Pair(be, SD.tiny(), 3, T, draft_b())
    accepted = []
    want = pair.check(three(pair), tag=f"T {T} B", on_step=lambda b, pos, c, g, a, m: accepted.append(a))
    assert 0 in accepted and T - 1 in accepted  # condition: a step that rejects everything, one that accepts everything
    for b in range(3):
        assert want[0][b, :COUNTS[b]].tolist() == streams[b][:COUNTS[b]] and np.all(want[0][b, COUNTS[b]:] == -1)
    for b in (0, 2):
        assert (want[2][b]["steps"], want[2][b]["drafted"], want[2][b]["accepted"]) == DRAFT_B[T]
    assert_draft_caches_are_in_step(pair, [[FIRSTS[b]] + streams[b][:COUNTS[b]] for b in range(3)], STARTS)
    pair.close()


# ── 3. two calls equal one, raggedly ───────────────────────────────────────────────────────────────────────────────────

def test_two_calls_equal_one_raggedly(hip_backend, oracle):
    """(10, 5, 24) tokens, then (14, 12, 0), then a third call that continues the sequence that idled: the streams are those of one
    call, the idle sequence's statistics are zero, and behind it all every sequence's draft cache is in step — the idled one's
    too. Then a call in which a sequence wants nothing from the start."""
    be, T = hip_backend, 4
    streams = [stream_of(be, oracle, 0, f, st) for f, st in zip(FIRSTS, STARTS)]
    pair = Pair(be, SD.tiny(), 3, T, draft_b())
    p = pair.prompt
    a = pair.check(three(pair, counts=[10, 5, N]), tag="first")[0]
    for b, n in enumerate([10, 5, N]):
        assert a[b, :n].tolist() == streams[b][:n] and np.all(a[b, n:] == -1)
    first2 = [int(a[0, 9]), int(a[1, 4]), int(a[2, N - 1])]
    start2 = [10, PROMPT_LEN + 5, N]
    hist2 = [[FIRST_AT_0] + a[0, :9].tolist(), p + [FIRST_AT_8] + a[1, :4].tolist(), [FIRST_AT_0] + a[2, :N - 1].tolist()]
    w2 = pair.check([BDM.Request(first2[b], start2[b], [14, 12, 0][b], history=hist2[b]) for b in range(3)], tag="second")
    assert a[0, :10].tolist() + w2[0][0, :14].tolist() == streams[0][:24]
    assert a[1, :5].tolist() + w2[0][1, :12].tolist() == streams[1][:17]
    assert np.all(w2[0][2] == -1) and w2[2][2] == ZERO and w2[1] == [14, 12, 0]
    first3 = [int(w2[0][0, 13]), int(w2[0][1, 11]), first2[2]]
    w3 = pair.check([BDM.Request(first3[b], [24, PROMPT_LEN + 17, N][b], [0, 0, 3][b]) for b in range(3)], tag="third")
    assert w3[0][2].tolist() == streams[2][N:N + 3] and np.all(w3[0][:2] == -1) and w3[2][0] == w3[2][1] == ZERO
    confirmed = [[FIRST_AT_0] + streams[0][:24], [FIRST_AT_8] + streams[1][:17], [FIRST_AT_0] + streams[2][:N + 3]]
    assert_draft_caches_are_in_step(pair, confirmed, STARTS)
    # a sequence that wants nothing from the start idles at its start position; all zero returns at once and touches nothing
    w4 = pair.check(three(pair, counts=[6, 0, 9]), tag="zero from the start")
    assert w4[0][0, :6].tolist() == streams[0][:6] and w4[0][2].tolist() == streams[2][:9] and np.all(w4[0][1] == -1) and w4[2][1] == ZERO
    before = (_dispatches(be, pair.s.handle), _dispatches(be, pair.d.handle))
    toks, produced, stats = pair.got(three(pair, counts=[0, 0, 0]))
    assert toks.shape == (3, 0) and produced.tolist() == [0, 0, 0] and stats == [ZERO] * 3
    assert (_dispatches(be, pair.s.handle), _dispatches(be, pair.d.handle)) == before
    pair.close()


# ── 4. int8 KV ─────────────────────────────────────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("kvq_t,kvq_d", [(32, 0), (0, 32)])
def test_int8_kv_equals_the_host_driven_pair(hip_backend, kvq_t, kvq_d):
    B, T = 2, 4
    pair = Pair(hip_backend, SD.tiny(), B, T, draft_b(), kvq_t=kvq_t, kvq_d=kvq_d, behind=())
    want = pair.check([BDM.Request([FIRST_INT8, FIRST_AT_0][b], 0, [N, 17][b]) for b in range(B)], tag=f"int8 {kvq_t} {kvq_d}")
    assert want[1] == [N, 17]
    pair.close()


# ── 5. the sampled verify step ─────────────────────────────────────────────────────────────────────────────────────────

KW = [dict(seed=1234, stream=0, **PARAMS["k40_p95"]), dict(seed=77, stream=3, **PARAMS["k256_p1"], **PEN4), dict(seed=9 << 32, stream=1, **PARAMS["k1"])]


def test_sampled_verify_per_sequence(hip_backend):
    """B = 3, T = 4, draft A: parameter sets k40_p95 / k256_p1 with PEN4 penalties / k1; sequence 0 gets a stop token that the
    reference shows falling inside a step; log-probabilities for sequence 1"""
    T = 4
    pair = Pair(hip_backend, SD.tiny(), 3, T)
    for seed in range(16):  # the stop token: from sequence 0's own reference stream, first occurrence, strictly inside a step's emission
        kw = [dict(k) for k in KW]
        kw[0]["seed"] = 1234 + seed
        steps = []
        ref = pair.want(three(pair, samplings=[S(**k) for k in kw]), on_step=lambda b, pos, c, g, a, m: steps.append((b, pos, m)))
        s0 = ref[0][0, :N].tolist()
        inside = [pos + k for b, pos, m in steps if b == 0 for k in range(m - 1)]  # (position pos + k holds candidate k: token index pos + k of the stream)
        at = next((i for i in inside if 3 <= i and s0[i] not in s0[:i]), None)
        if at is not None:
            break
    else:
        pytest.fail("no reference stream emits a new token inside a step")
    plain = pair.want(three(pair, samplings=[S(**dict(k, repeat_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0)) for k in kw]))
    assert ref[1] == COUNTS and len(set(s0)) > 3 and ref[0][1].tolist() != plain[0][1].tolist()  # conditions: it samples; the penalties matter
    accepted = []
    pair.want(three(pair, samplings=[S(**k) for k in kw]), on_step=lambda b, pos, c, g, a, m: accepted.append(a))
    assert any(0 < a < T - 1 for a in accepted), accepted  # condition: a step accepted in part
    pair.check(three(pair, samplings=[S(**k) for k in kw]), tag="sampled")
    kw[0]["stop"] = [s0[at]]
    want = pair.check(three(pair, samplings=[S(**k) for k in kw]), logprobs=[False, True, False], tag="stop + logprobs")
    assert want[1] == [at + 1, COUNTS[1], COUNTS[2]]  # sequence 0 ends at its stop token, inside a step; the others finish
    assert want[0][0, :at + 1].tolist() == s0[:at + 1] and np.all(want[0][0, at + 1:] == -1)
    assert want[0][1].tolist() == ref[0][1].tolist() and want[0][2].tolist() == ref[0][2].tolist()
    lp = bits(pair.got(three(pair, samplings=[S(**k) for k in kw]), logprobs=[False, True, False])[3])
    assert not np.any(lp[1, :COUNTS[1]] == NAN_WORD) and np.all(lp[1, COUNTS[1]:] == NAN_WORD) and np.all(lp[0] == NAN_WORD)
    pair.close()


def test_top_k_1_equals_the_greedy_form(hip_backend):
    pair = Pair(hip_backend, SD.tiny(), 3, 4, draft_b())
    g = pair.got(three(pair))
    k = pair.got(three(pair, samplings=[S(seed=b + 1, stream=b, **PARAMS["k1"]) for b in range(3)]))
    assert k[0].tolist() == g[0].tolist() and k[1].tolist() == g[1].tolist() == COUNTS and k[2] == g[2]
    pair.close()


# ── 6. Llama-2-7B dimensions ───────────────────────────────────────────────────────────────────────────────────────────

def test_l7_dimensions_equal_the_host_driven_pair(hip_backend):
    """one layer each at Llama-2-7B dimensions, B = 2, T = 2, 8 tokens. The host-driven pair is the only reference
    (tests/test_hip_spec_decode.py says why the tie condition cannot hold here)."""
    B, T, n = 2, 2, 8
    pair = Pair(hip_backend, l7cfg(1), B, T, l7cfg(1), behind=(), threads=16)
    want = pair.check([BDM.Request([20000, 123][b], 0, n) for b in range(B)], tag="l7")
    assert want[1] == [n, n]
    pair.close()


# ── 7. the pair's graphs, the profile ──────────────────────────────────────────────────────────────────────────────────

def test_pair_graphs_follow_the_draft_and_the_profile_counts_both_programs(hip_backend):
    be, T, B = hip_backend, 4, 3
    pair = Pair(be, SD.tiny(), B, T, behind=())
    s, da = pair.s, pair.d
    db, dbm = draft_batch_session(be, B, draft_b())
    firsts, starts, counts = [FIRST_AT_0, FIRST_AT_8, FIRST_AT_0], [0, 0, 0], [N, 17, N]
    sps = [S(seed=b + 5, stream=b, **PARAMS["k40_p95"]) for b in range(B)]

    def delta(sess, call):
        """-> (launches, executions) the call added to the session's runtime profile, and its result"""
        b = _dispatches(be, sess.handle)
        out = call()
        a = _dispatches(be, sess.handle)
        assert not be.last_error(), be.last_error()
        return a[0] - b[0], a[1] - b[1], out

    def run(d):
        g = s.resident_decode_batch_speculative_model(d, firsts, starts, counts)
        k = s.resident_decode_batch_speculative_model(d, firsts, starts, counts, samplings=sps)
        assert not be.last_error(), be.last_error()
        return (g[0].tolist(), g[1].tolist(), g[2], k[0].tolist(), k[1].tolist(), k[2])

    def others():
        n = s.resident_decode_batch_speculative(firsts, starts, counts)
        k = s.resident_decode_batch_speculative_sampled(firsts, starts, counts, sps)
        p = db.resident_decode_batch(firsts, starts, 6)
        assert not be.last_error(), be.last_error()
        return (n[0].tolist(), n[1], k[0].tolist(), k[1].tolist(), k[2], p.tolist())

    first_a, first_b = run(da), run(db)
    assert first_a[2] == [full(T, n) for n in counts] and first_b[2] != first_a[2]  # condition: the statistics tell the two drafts apart
    assert run(da) == first_a
    first_others = others()
    db.close(), dbm.close()  # freed: a new draft B may land at the old address
    db, dbm = draft_batch_session(be, B, draft_b())
    assert run(db) == first_b
    for _ in range(2):  # interleaved with the other loops of either program: nothing is invalidated
        assert others() == first_others
        assert run(db) == first_b
        assert run(da) == first_a
    db.resident_setup(be)  # set up again: the pair re-captures
    assert run(db) == first_b

    # the profile. One step of the batched decode loop is [batched prep] [plan] [pick x 2]: plan + 3 launches
    plan_d = delta(db, lambda: db.resident_decode_batch(firsts, starts, 1))[0] - 3
    # zgml_hip_resident_decode_batch_speculative: [draft] [prep] [plan] [stage 1] [accept] per step that ran; its sampled form one more
    launches, ran, _ = delta(s, lambda: s.resident_decode_batch_speculative(firsts, starts, counts))
    assert ran > 0 and launches % ran == 0
    plan_t = launches // ran - 4
    launches, ran, _ = delta(s, lambda: s.resident_decode_batch_speculative_sampled(firsts, starts, counts, sps))
    assert launches == ran * (plan_t + 5)
    # the pair: the target plan + 3 + tail, the draft T x (plan + 3)
    for samplings, tail in ((None, 1), (sps, 2)):
        before_d = _dispatches(be, db.handle)
        launches, ran, _ = delta(s, lambda: s.resident_decode_batch_speculative_model(db, firsts, starts, counts, samplings=samplings))
        after_d = _dispatches(be, db.handle)
        assert ran > 0 and launches == ran * (plan_t + 3 + tail)
        assert (after_d[0] - before_d[0], after_d[1] - before_d[1]) == (ran * T * (plan_d + 3), ran * T)
    # ... and the n-gram batched step afterwards counts what it counted
    launches, ran, _ = delta(s, lambda: s.resident_decode_batch_speculative(firsts, starts, counts))
    assert launches == ran * (plan_t + 4)
    db.close(), dbm.close(), pair.close()

    # the single-sequence call with a draft model launches what it launched: plan + 3 + 1 and T x (plan + 3)
    ss, sm = SD.spec_session(be, SD.tiny(), T)
    sd, sdm = draft_session(be, like=sm)
    p_t = delta(ss, lambda: ss.resident_prefill(SD.prompt(SD.tiny(), T), 0))[0] - 3
    p_d = delta(sd, lambda: sd.resident_prefill([1], 0))[0] - 3
    before_d = _dispatches(be, sd.handle)
    launches, ran, (_, stats) = delta(ss, lambda: ss.resident_decode_speculative_model(sd, FIRST_AT_0, 0, N))
    after_d = _dispatches(be, sd.handle)
    assert stats == full(T, N) and ran == N // T and launches == ran * (p_t + 4)
    assert (after_d[0] - before_d[0], after_d[1] - before_d[1]) == (ran * T * (p_d + 3), ran * T)
    for x in (sd, sdm, ss, sm):
        x.close()


# ── 8. refusals ────────────────────────────────────────────────────────────────────────────────────────────────────────

def test_refusals_enqueue_nothing_and_leave_both_programs_usable(hip_backend):
    be, B, T = hip_backend, 3, 4
    cfg = SD.tiny()
    hip, V, Smax = capi.load_hip(), cfg.vocab_size, 32
    fns = llama.hip_backend_fns(be)
    s, m = batch_session(be, cfg, B, T)
    d, dm = draft_batch_session(be, B, draft_b(max_seq=Smax))  # the smaller cache of the pair
    call = s.resident_decode_batch_speculative_model
    firsts, zeros, fours = [FIRST_AT_0, 1, 2], [0, 0, 0], [4, 4, 4]
    good = call(d, firsts, zeros, [8, 3, 8])
    before = (_dispatches(be, s.handle), _dispatches(be, d.handle))
    kept = []

    def refused(fn, text):
        with pytest.raises(RuntimeError, match=text):
            fn()
        hip.zgml_hip_clear_error(be.ctx)
        assert (_dispatches(be, s.handle), _dispatches(be, d.handle)) == before, text

    # of the requests and the target, as zgml_hip_resident_decode_batch_speculative: the sequence is named
    refused(lambda: call(d, [1, V, 1], zeros, fours), r"sequence 1\).*token out of range")
    refused(lambda: call(d, firsts, [0, 0, 2], fours, histories=[None, None, [1, V]]), r"sequence 2\).*token out of range")
    refused(lambda: call(d, firsts, [0, 3, 0], fours, histories=[None, [1, 2], None]), r"sequence 1\).*n_history")
    refused(lambda: call(d, firsts, [cfg.max_seq_len - T - 3, 0, 0], fours), r"sequence 0\).*exceeds max_seq")
    refused(lambda: d.resident_decode_batch_speculative_model(s, firsts, zeros, fours), "one column per sequence")  # (the target must hold T >= 2 columns)
    plain, pm = draft_session(be, draft_b())
    out, u32 = np.zeros((B, 4), np.int64), lambda a: np.ascontiguousarray(a, np.uint32).ctypes.data_as(C.POINTER(C.c_uint32))

    def plain_target():  # (no BatchSession to call it on: the entry point itself)
        if hip.zgml_hip_resident_decode_batch_speculative_model(be.ctx, plain.handle, d.handle, u32(firsts), u32(zeros), u32(fours), 4, None, None, None,
                                                                out.ctypes.data, None, None) != 0:
            raise RuntimeError(be.last_error())
    refused(plain_target, "not a batched program")
    # ... with sampling, as the sampled form
    ok = [S(seed=1, **PARAMS["k40_p95"])] * 2
    refused(lambda: call(d, firsts, zeros, fours, samplings=ok + [S(temperature=0.0, top_k=4, top_p=1.0)]), r"sequence 2\).*temperature")
    refused(lambda: call(d, firsts, zeros, fours, samplings=ok + [S(recent=[], seed=1, **PARAMS["k40_p95"], **PEN4)]), "recent must be NULL")
    # of the draft
    refused(lambda: call(None, firsts, zeros, fours), "no draft")
    refused(lambda: call(s, firsts, zeros, fours), "target program itself")
    be2 = Backend(0)
    o, om = draft_batch_session(be2, B, draft_b())
    refused(lambda: call(o, firsts, zeros, fours), "another context")
    o.close(), om.close(), be2.close()
    bare, bm = draft_batch_session(be, B, draft_b(), setup=False)
    refused(lambda: call(bare, firsts, zeros, fours), "no resident set-up")
    refused(lambda: call(plain, firsts, zeros, fours), "plain plan")
    two, tm = batch_session(be, cfg, B, 2)
    refused(lambda: call(two, firsts, zeros, fours), "tokens_per_seq = 1")
    fewer, fm = draft_batch_session(be, B - 1, draft_b())
    refused(lambda: call(fewer, firsts, zeros, fours), "another n_seqs")
    other = draft_b()
    other.vocab_size = V // 2
    ov, ovm = draft_batch_session(be, B, other)
    refused(lambda: call(ov, firsts, zeros, fours), "vocabulary")
    sh, shm = draft_batch_session(be, B, draft_b())
    pt = capi.ShardPointC(shm.program.n_ops, shm.buf("logits"), 0, 0, V)
    assert hip.zgml_hip_shard_attach(be.ctx, sh.handle, C.byref(pt), 1, shm.buf("logits"), V) == 0
    refused(lambda: call(sh, firsts, zeros, fours), "draft is a sharded")
    st, stm = batch_session(be, cfg, B, T)
    pt = capi.ShardPointC(stm.program.n_ops, stm.buf("logits"), 0, 0, V)
    assert hip.zgml_hip_shard_attach(be.ctx, st.handle, C.byref(pt), 1, stm.buf("logits"), V) == 0
    refused(lambda: st.resident_decode_batch_speculative_model(d, firsts, zeros, fours), "target is a sharded")
    # the bound on the draft: start + n + T = 33 > 32 for sequence 1
    refused(lambda: call(d, firsts, [0, Smax - T - 3, 0], fours), r"sequence 1\).*draft's max_seq")
    # a constraint on any sequence of either program
    class_of, nxt = np.zeros(V, np.uint16), np.zeros((1, 1), np.uint16)  # one state, every token allowed
    con = be.constraint_create(class_of, nxt)
    d.set_constraint(con, 0, 2)
    refused(lambda: call(d, firsts, zeros, fours), "constraint is attached to the draft")
    d.set_constraint(None, 0, 2)
    s.set_constraint(con, 0, 1)
    refused(lambda: call(d, firsts, zeros, fours), "constraint is attached")
    s.set_constraint(None, 0, 1)
    be.constraint_free(con)
    # the n-gram siblings keep refusing mode > 1
    opt = (capi.SpecDecodeC * B)()
    for b in range(B):
        opt[b].mode = 2
    assert hip.zgml_hip_resident_decode_batch_speculative(be.ctx, s.handle, u32(firsts), u32(zeros), u32(fours), 4, opt, out.ctypes.data, None) == -1
    assert "mode must be 0 or 1" in be.last_error()
    hip.zgml_hip_clear_error(be.ctx)
    # no tokens wanted: 0, nothing touched
    toks, produced, stats = call(d, firsts, zeros, 0)
    assert toks.shape == (B, 0) and stats == [ZERO] * B
    assert (_dispatches(be, s.handle), _dispatches(be, d.handle)) == before
    # the allowed edge of the smaller cache: start + n + T == 32
    toks, produced, _ = call(d, firsts, [0, Smax - T - 4, 0], fours)
    assert produced.tolist() == fours and not be.last_error(), be.last_error()
    # ... and both programs are usable: the first call again
    again = call(d, firsts, zeros, [8, 3, 8])
    assert again[0].tolist() == good[0].tolist() and again[2] == good[2] and not be.last_error()
    for x in (d, dm, s, m, plain, pm, bare, bm, two, tm, fewer, fm, ov, ovm, sh, shm, st, stm):
        x.close()

