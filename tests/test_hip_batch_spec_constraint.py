"""Constrained speculative decode under batching on the MI355X (zgml_hip_resident_decode_batch_speculative_constrained): B sequences
on a batched plan with Ts columns per sequence, every one running the constrained verify loop of
zgml_hip_resident_decode_speculative_constrained on the device with its own automaton and state — or none —, its own parameter set,
stream, seed, stop set, penalties and `logprobs` word.

THE REFERENCE everywhere is the SAME batched plan driven from the host in lock-step with the device loop
(tests/batch_spec_constraint_model.py), as in tests/test_hip_batch_spec_sampled.py: per step the candidates of all B sequences after
each sequence's own pass, ONE BatchSession.step over the B * Ts tokens through the vtable, all rows downloaded, row b * Ts + j picked
on the CPU by zgml_amd/csrc/sample.h (tests/cpp/constraint_probe.cpp: c_constraint_sample) under the state the model gave that row —
the sampled probes for a sequence without an automaton —, the acceptance per sequence. Same kernels, same inputs, same step
grouping: exact equality of tokens, counts, statistics, final states and log-probability bits, no tolerance.

Every reference is computed from the reference alone; its preconditions — the stream holds forced runs, the free picks do sample,
"wrong" drafts are wrong, a dead end is reached where meant — are asserted on it before the device is asked."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

from zgml_amd import capi, llama
from tests import batch_spec_constraint_model as BCM
from tests import spec_constraint_model as SCM
from tests import test_hip_batch_spec_sampled as BS
from tests import test_hip_spec_decode as SD
from tests.test_constraint_host import Dfa, FORBIDDEN
from tests.test_hip_batch_spec_decode import batch_session
from tests.test_hip_constraint import hashed_classes, seeded_dfa
from tests.test_hip_l7dims import l7cfg
from tests.test_spec_constraint_host import chain_dfa, template_dfa

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
S = capi.SamplingC.of
u16 = np.uint16
u32p = C.POINTER(C.c_uint32)
V = 512  # the tiny preset's vocabulary
N, PROMPT_LEN, FIRST_AT_0, FIRST_AT_8 = SD.N, SD.PROMPT_LEN, SD.FIRST_AT_0, SD.FIRST_AT_8
FIRSTS, STARTS, COUNTS, KW, PEN, ZERO, NAN_WORD = BS.FIRSTS, BS.STARTS, BS.COUNTS, BS.KW, BS.PEN, BS.ZERO, BS.NAN_WORD
TEMPLATE, TEMPLATE_FREE, TEMPLATE_LITS = template_dfa(V, [0, 1, 0, 3, 0, 6], seed=21)  # literal runs of 1, 3 and 6 forced tokens between free states
SEEDED = seeded_dfa(11, V)
FORMS = ["perfect", "ngram", "wrong_everywhere", "none"]


def drafts_for(form, stream):
    return [] if form == "none" else SD.drafts_of(form, stream, V)


class Pair(BS.Pair):
    """BS.Pair — the device session and the reference session over one batched plan — with the requests' automata: `want` replays
    them through the constrained lock-step model, `got` attaches them to the device session's sequences and asks the device loop"""

    def __init__(self, *a, **kw):
        BS.Pair.__init__(self, *a, **kw)
        self.handles = {}  # id(dfa) -> (the uploaded constraint, the dfa)

    def want(self, rqs, max_tokens=None, seqs_out=None):
        return BCM.lockstep(lambda toks, pos: self.host.step(toks, pos)[1], self.Ts, rqs, max_tokens=max_tokens, seqs_out=seqs_out)

    def attach(self, rqs):
        for b, rq in enumerate(rqs):
            if rq.dfa is None:
                self.s.set_constraint(None, seq=b)
                continue
            if id(rq.dfa) not in self.handles:
                self.handles[id(rq.dfa)] = (self.be.constraint_create(rq.dfa.class_of, rq.dfa.next), rq.dfa)
            self.s.set_constraint(self.handles[id(rq.dfa)][0], rq.state, seq=b)

    def got(self, rqs, logprobs=None):
        """-> the device call's results and the sequences' states afterwards (-1: none attached)"""
        self.attach(rqs)
        out = self.s.resident_decode_batch_speculative_constrained([r.first for r in rqs], [r.start for r in rqs], [r.n for r in rqs], [r.sampling for r in rqs],
                                                                   histories=[r.history for r in rqs], drafts=[r.drafts for r in rqs], logprobs=logprobs)
        assert not self.be.last_error(), self.be.last_error()
        return out + ([self.s.constraint_state(seq=b) for b in range(self.B)],)

    def check(self, rqs, logprobs=None, tag="", seqs_out=None):
        """the device equals the replay of the same requests -> the reference"""
        want = self.want(rqs, seqs_out=seqs_out)
        return self.compare(want, self.got(rqs, logprobs), logprobs, tag)

    def compare(self, want, got, logprobs=None, tag=""):
        print(tag, "produced", want[1], "stats", got[2], "states", got[-1])
        assert got[0].tolist() == want[0].tolist(), tag
        assert np.asarray(got[1]).tolist() == want[1] and got[2] == want[2], (tag, got[1], want[1], got[2], want[2])
        assert got[-1] == want[4], (tag, got[-1], want[4])
        if logprobs is not None:
            flags = [bool(logprobs)] * self.B if isinstance(logprobs, bool) else list(logprobs)
            for b in range(self.B):
                row = BS.bits(want[3][b]) if flags[b] else np.full(want[3].shape[1], NAN_WORD, np.uint32)
                print(tag, "sequence", b, "log-probability bits differing:", int(np.sum(BS.bits(got[3][b]) != row)))
                assert BS.bits(got[3][b]).tolist() == row.tolist(), (tag, b)
        return want

    def close(self):
        for b in range(self.B):
            self.s.set_constraint(None, seq=b)
        for handle, _ in self.handles.values():
            self.be.constraint_free(handle)
        assert not self.be.last_error(), self.be.last_error()
        BS.Pair.close(self)


def three(pair, kw=KW, counts=COUNTS, drafts=(None, None, None), dfas=(TEMPLATE, SEEDED, None), states=(0, 1, 0), hists=None):
    """sequence 0 the template from position 0, sequence 1 behind the admitted prompt with a seeded automaton without forced states,
    sequence 2 with nothing attached"""
    hists = [None, pair.prompt, None] if hists is None else hists
    return [BCM.Request(FIRSTS[b], STARTS[b], counts[b], S(**kw[b]), history=hists[b], drafts=drafts[b], dfa=dfas[b], state=states[b]) for b in range(3)]


def streams_of(pair, kw=KW, seqs_out=None, **more):
    """every sequence's stream from a replay without any draft, Ts - 1 tokens longer than its count: perfect drafts exist for the
    last step"""
    long = [n + pair.Ts - 1 for n in COUNTS]
    toks, produced, _, _, _ = pair.want(three(pair, kw, counts=long, drafts=([], [], []), **more), seqs_out=seqs_out)
    assert produced == long  # precondition: the walks go on
    return [toks[b, :long[b]].tolist() for b in range(3)]


# ── 1. a mixed batch ───────────────────────────────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("pen", [False, True], ids=["plain", "penalties"])
@pytest.mark.parametrize("Ts", [2, 4, 5])
def test_mixed_batch_equals_the_lockstep_replay(hip_backend, Ts, pen):
    """B = 3: the template (literal runs of 1, 3 and 6), a seeded automaton without forced states behind the admitted prompt, and an
    unattached sequence, each with its own parameter set; penalties on for sequences 0 and 2. A select that took rows[0] or
    params[0] for every sequence fails here"""
    pair = Pair(hip_backend, SD.tiny(), 3, Ts)
    kw = [dict(KW[0], **PEN), dict(KW[1]), dict(KW[2], **PEN)] if pen else KW
    seqs = []
    streams = streams_of(pair, kw, seqs_out=seqs)
    frc0, lits = seqs[0].frc, set(sum(TEMPLATE_LITS, []))
    assert all(f == SCM.NO_FORCED for f in seqs[1].frc) and sum(f != SCM.NO_FORCED for f in frc0) == 10  # preconditions on the automata
    assert sum(t in lits for t in streams[0]) >= 8  # the stream holds forced runs
    free0 = [pick for st, pick in seqs[0].seen.values() if frc0[st] == SCM.NO_FORCED]
    assert len(set(free0)) > 3 and len(set(streams[1])) > 3  # the free picks do sample
    assert seqs[0].stats["steps"] < len(streams[0])  # forced runs are jumped over without any draft
    one_stream = True
    for rot in range(4):
        fb = [FORMS[(b + rot) % 4] for b in range(3)]
        drafts = [drafts_for(fb[b], streams[b]) for b in range(3)]
        for b in range(3):
            if fb[b] == "wrong_everywhere":
                assert all(d != t for d, t in zip(drafts[b], streams[b]))  # precondition
        want = pair.check(three(pair, kw, drafts=drafts), tag=f"Ts {Ts} {fb}")
        for b in range(3):
            assert want[1][b] == COUNTS[b] and np.all(want[0][b, COUNTS[b]:] == -1)
            if fb[b] == "perfect":
                assert want[2][b]["steps"] == -(-COUNTS[b] // Ts)
            one_stream = one_stream and want[0][b, :COUNTS[b]].tolist() == streams[b][:COUNTS[b]]
        if BS.closed_form(fb[2], COUNTS[2], Ts):  # the unattached sequence: the sampled call's closed forms, `drafted` its real drafts alone
            assert want[2][2] == BS.closed_form(fb[2], COUNTS[2], Ts)
        assert want[4][2] == -1
    print(f"Ts {Ts}: the four draft forms gave one stream per sequence: {one_stream}")
    pair.close()


# ── 2. nothing attached: the sampled batched call ──────────────────────────────────────────────────────────────────────

def test_nothing_attached_is_the_sampled_batched_call(hip_backend):
    be, Ts = hip_backend, 4
    pair = Pair(be, SD.tiny(), 3, Ts)
    s, hists = pair.s, [None, pair.prompt, None]
    for kw in (KW, [dict(KW[0], **PEN), dict(KW[1]), dict(KW[2], **PEN)]):
        sps = [S(**k) for k in kw]
        for drafts in (None, [[], [], []]):
            for lp in (None, [True, False, True]):
                d0 = SD._dispatches(be, s.handle)
                a = s.resident_decode_batch_speculative_sampled(FIRSTS, STARTS, COUNTS, sps, histories=hists, drafts=drafts, logprobs=lp)
                d1 = SD._dispatches(be, s.handle)
                b = s.resident_decode_batch_speculative_constrained(FIRSTS, STARTS, COUNTS, sps, histories=hists, drafts=drafts, logprobs=lp)
                d2 = SD._dispatches(be, s.handle)
                assert not be.last_error(), be.last_error()
                assert b[0].tolist() == a[0].tolist() and b[1].tolist() == a[1].tolist() and b[2] == a[2]
                assert lp is None or BS.bits(b[3]).tolist() == BS.bits(a[3]).tolist()
                steps = d1[1] - d0[1]
                assert steps > 0 and d2[1] - d1[1] == steps and d2[0] - d1[0] == d1[0] - d0[0]  # the same steps of the same launches
    pair.close()


def test_graphs_are_the_sampled_call_s_with_nothing_attached_and_its_own_with_an_automaton():
    """A fresh process with the graph dump on names every graph it captures: a detached constrained call captures none beside the
    sampled call's, an attached one captures the batched constrained-rows forms, and nothing is captured twice"""
    worker = Path(__file__).parent / "batch_spec_constraint_graphs_worker.py"
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([sys.executable, str(worker)], capture_output=True, text=True, timeout=280, cwd=ROOT, env=dict(os.environ, ZGML_HIP_GRAPH_DUMP=tmp))
    assert r.returncode == 0 and "BATCH_SPEC_CONSTRAINT_GRAPHS_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    phases, at = {}, None  # (the worker names its phases on stderr, where the library names its graphs)
    for line in r.stderr.splitlines():
        if line.startswith("PHASE "):
            at = phases.setdefault(line.split()[1], [])
        named = re.match(r"\[zgml_hip\] graph (resident\w+):", line)
        if named and at is not None:
            at.append(named.group(1))
    print(phases)
    assert phases["sampled"] == ["resident_batch_spec_sampled"]
    assert phases["detached"] == []  # same graph slot: nothing new
    assert phases["attached"] == ["resident_batch_spec_constrained_rows"]
    assert phases["attached_logprobs"] == ["resident_batch_spec_constrained_rows_logprobs"]
    assert phases["greedy"] == ["resident_batch_spec"]
    assert phases["again"] == []  # every call twice more, interleaved, once every table has its size: all replays, no call drops another's graph


# ── 3. independence ────────────────────────────────────────────────────────────────────────────────────────────────────

def test_a_sequence_does_not_depend_on_its_neighbours(hip_backend):
    Ts = 4
    pair = Pair(hip_backend, SD.tiny(), 3, Ts)
    chain = chain_dfa(V, 7)
    a = three(pair)
    b = three(pair, kw=[KW[0], dict(KW[2], **PEN), dict(KW[1], seed=5)], dfas=(TEMPLATE, chain, TEMPLATE), states=(0, 2, 3), counts=[N, 9, 11],
              drafts=(None, [1] * 40, []))
    got_a = pair.got(a)
    pair.compare(pair.want(a), got_a, tag="neighbours a")
    got_b = pair.got(b)
    pair.compare(pair.want(b), got_b, tag="neighbours b")
    assert got_b[1][1] == 4  # (precondition of the case: the neighbour dead-ends)
    assert got_a[0][0].tolist() == got_b[0][0, :N].tolist() and got_a[1][0] == got_b[1][0] and got_a[2][0] == got_b[2][0] and got_a[-1][0] == got_b[-1][0]
    pair.close()


# ── 4. dead ends ───────────────────────────────────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("state1,k", [(0, 6), (6, 0)], ids=["after_6", "at_the_first_pick"])
def test_a_dead_end_finishes_its_sequence_and_the_others_go_on(hip_backend, state1, k):
    Ts = 4
    pair = Pair(hip_backend, SD.tiny(), 3, Ts)
    chain = chain_dfa(V, 7)  # every token is allowed, six times; state 6 allows none
    for drafts1 in (None, [], [3] * 40):
        seqs = []
        rqs = three(pair, dfas=(TEMPLATE, chain, None), states=(0, state1, 0), drafts=(None, drafts1, None))
        want = pair.want(rqs, seqs_out=seqs)
        # preconditions, on the reference: the dead end is reached where meant, by sequence 1 alone
        assert want[1] == [N, k, N] and seqs[1].dead_end and not seqs[0].dead_end and not seqs[2].dead_end and want[4] == [want[4][0], 6, -1]
        assert np.all(want[0][1, k:] == -1) and np.all(want[0][1, :k] >= 0)
        got = pair.got(rqs)  # (returns 0 and leaves no error on the context: got asserts it)
        pair.compare(want, got, tag=f"dead end after {k}, drafts {drafts1 if drafts1 is None else len(drafts1)}")
        assert pair.s.constraint_state(seq=1) == 6
    # ... and the next call, from a live state, works
    pair.check(three(pair, dfas=(TEMPLATE, chain, None), states=(0, 1, 0), counts=[N, 5, N]), tag="after the dead end")
    pair.close()


# ── 5. state across calls, stop tokens ─────────────────────────────────────────────────────────────────────────────────

def test_two_ragged_calls_equal_one_and_a_stop_token_advances_the_state(hip_backend):
    Ts = 4
    pair = Pair(hip_backend, SD.tiny(), 3, Ts)
    one = pair.check(three(pair), tag="one call")
    cut = [10, 17, 3]  # sequence 1 has everything after the first call and idles through the second
    a = pair.check(three(pair, counts=cut), tag="first call")
    rest = [COUNTS[b] - cut[b] for b in range(3)]
    hists = [([None, pair.prompt, None][b] or []) + [FIRSTS[b]] + a[0][b, :cut[b] - 1].tolist() for b in range(3)]
    rq2 = [BCM.Request(int(a[0][b, cut[b] - 1]), STARTS[b] + cut[b], rest[b], S(**KW[b]), history=hists[b], dfa=(TEMPLATE, SEEDED, None)[b], state=max(a[4][b], 0))
           for b in range(3)]
    want2 = pair.want(rq2)
    # the device carries the states itself: the second call does not attach again
    got2 = pair.s.resident_decode_batch_speculative_constrained([r.first for r in rq2], [r.start for r in rq2], rest, [r.sampling for r in rq2],
                                                                histories=hists)
    pair.compare(want2, got2 + ([pair.s.constraint_state(seq=b) for b in range(3)],), tag="second call")
    for b in range(3):
        assert a[0][b, :cut[b]].tolist() + want2[0][b, :rest[b]].tolist() == one[0][b, :COUNTS[b]].tolist() and want2[4][b] == one[4][b], b
    assert want2[2][1] == ZERO
    # a stop token of sequence 0 inside a step: it cuts, advances the state, and the sequence idles while the others go on
    stream = one[0][0].tolist()
    at = next(i for i in range(2, N) if stream[i] not in stream[:i] and i % Ts != Ts - 1)
    kw = [dict(KW[0], stop=[stream[at]]), KW[1], KW[2]]
    for drafts0 in (stream, [], None):
        want = pair.check(three(pair, kw, drafts=(drafts0, None, None)), tag="stop")
        assert want[1] == [at + 1, 17, N] and want[0][0, :at + 1].tolist() == stream[:at + 1] and np.all(want[0][0, at + 1:] == -1)
        state = 0
        for t in stream[:at + 1]:
            state = TEMPLATE.advance(state, t)
        assert want[4][0] == state  # over the stop token too
        assert want[0][1].tolist() == one[0][1].tolist() and want[0][2].tolist() == one[0][2].tolist()
    pair.close()


# ── 6. forced runs ─────────────────────────────────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("Ts", [2, 4, 5])
def test_a_pure_forced_run_takes_ceil_L_plus_1_over_Ts_steps(hip_backend, Ts):
    """From the first literal state of a run of L, L + 1 tokens — the run and the free pick behind it — without any draft: every
    step emits Ts tokens, the forced tokens placed on pads are what `drafted` counts, and all of them are accepted"""
    pair = Pair(hip_backend, SD.tiny(), 3, Ts, behind=())
    runs = [6, 3]
    dfas = [template_dfa(V, [L], seed=40 + L)[0] for L in runs] + [None]
    counts = [runs[0] + 1, runs[1] + 1, 5]
    rqs = [BCM.Request(FIRST_AT_0, 0, counts[b], S(**KW[b]), drafts=[], dfa=dfas[b], state=1 if dfas[b] is not None else 0) for b in range(3)]
    want = pair.want(rqs)
    for b, L in enumerate(runs):  # on the reference ...
        steps = -(-(L + 1) // Ts)
        assert want[1][b] == L + 1 and want[2][b] == {"steps": steps, "drafted": L + 1 - steps, "accepted": L + 1 - steps}, (b, want[2][b])
        assert want[4][b] == 1  # through the free state, at the run's first literal again
    assert want[2][2]["drafted"] == 0  # nothing is placed for the unattached sequence
    pair.compare(want, pair.got(rqs), tag=f"forced runs, Ts {Ts}")  # ... then on the device
    pair.close()


# ── 7. the edges of the tables ─────────────────────────────────────────────────────────────────────────────────────────

def test_table_edges_side_by_side(hip_backend):
    """n_classes = 8192 — the staged state row fills its LDS exactly — with several thousand states, beside n_classes = 1 with
    n_states = 1, beside a sequence whose only allowed class has no tokens"""
    Ts = 4
    pair = Pair(hip_backend, SD.tiny(), 3, Ts, behind=())
    rng = np.random.default_rng(17)
    n_states, n_classes = 3000, 8192
    class_of = rng.permutation(n_classes)[:V].astype(u16)
    class_of[:2] = [n_classes - 1, 0]  # the last and the first word of the staged row are read
    nxt = rng.integers(0, n_states, (n_states, n_classes), dtype=u16)
    nxt[rng.integers(0, 2, (n_states, n_classes), dtype=np.uint8) == 1] = FORBIDDEN
    big = Dfa(class_of, nxt)
    assert all(big.allowed(s).sum() > 100 for s in range(0, n_states, 97))  # no dead end on the way
    everything = Dfa(np.zeros(V, u16), np.zeros((1, 1), u16))
    empty = Dfa(np.zeros(V, u16), np.array([[FORBIDDEN, 0]], u16))  # class 1 is allowed and has no tokens
    assert not empty.allowed(0).any()
    n = 13
    for drafts in (None, []):
        seqs = []
        rqs = [BCM.Request(FIRST_AT_0, 0, n, S(**KW[b]), drafts=drafts, dfa=(big, everything, empty)[b], state=(2999, 0, 0)[b]) for b in range(3)]
        want = pair.want(rqs, seqs_out=seqs)
        assert want[1] == [n, n, 0] and seqs[2].dead_end and len({st for st, _ in seqs[0].seen.values()}) > 3
        picked = {int(class_of[t]) for t in want[0][0, :n]}
        print("classes of sequence 0's tokens:", sorted(picked))
        pair.compare(want, pair.got(rqs), tag="table edges")
    pair.close()


# ── 8. more than one slice per row ─────────────────────────────────────────────────────────────────────────────────────

def test_l7_dimensions_every_row_is_masked_with_its_own_sequence_s_state(hip_backend):
    """Two layers at Llama-2-7B dimensions, B = 2, Ts = 4, 12 tokens: vocab 32000 is 18 slices per row. Sequence 0's consecutive
    states allow DISJOINT hashed classes; sequence 1 walks a seeded automaton over other classes"""
    B, Ts, n = 2, 4, 12
    base = llama.Model(l7cfg(2), llama.Q4_0, threads=16)
    pair = Pair(hip_backend, base.cfg, B, Ts, like=base, behind=(), threads=16)
    vocab = base.cfg.vocab_size
    nxt = np.full((4, 8), FORBIDDEN, u16)
    for st in range(4):
        nxt[st, 2 * st] = nxt[st, 2 * st + 1] = (st + 1) % 4
    dfas = [Dfa(hashed_classes(vocab, 8), nxt), seeded_dfa(7, vocab)]
    firsts = [20000, 4321]
    kw = [dict(temperature=1.0, top_k=40, top_p=0.9, seed=31, stream=4), dict(temperature=1.3, top_k=256, top_p=1.0, seed=32, stream=5)]

    def rqs(drafts, count=n):
        return [BCM.Request(firsts[b], 0, count, S(**kw[b]), drafts=drafts[b], dfa=dfas[b], state=(0, 1)[b]) for b in range(B)]

    ref = pair.want(rqs([[], []], n + Ts - 1))
    assert ref[1] == [n + Ts - 1] * 2
    right = [ref[0][b].tolist() for b in range(B)]
    wrong = [[(t + 8) % vocab if i in (2, 7) else t for i, t in enumerate(r)] for r in right]
    for drafts in ([None, None], right, [wrong[0], None], [right[0], wrong[1]]):
        want = pair.check(rqs(drafts), logprobs=[False, True], tag="l7")
        assert want[1] == [n, n] and want[4][0] == n % 4
    pair.close(), base.close()


# ── 9. int8 KV ─────────────────────────────────────────────────────────────────────────────────────────────────────────

def test_int8_kv(hip_backend):
    B, Ts = 3, 4
    pair = Pair(hip_backend, SD.tiny(), B, Ts, kvq=32, behind=())
    firsts, counts = [SD.FIRST_INT8, FIRST_AT_0, FIRST_AT_0], [N, 17, 11]

    def rqs(drafts, extra=0):
        return [BCM.Request(firsts[b], 0, counts[b] + extra, S(**KW[b]), drafts=drafts[b], dfa=(TEMPLATE, SEEDED, None)[b], state=(0, 1, 0)[b]) for b in range(B)]

    long = pair.want(rqs([[], [], []], Ts - 1))
    assert long[1] == [c + Ts - 1 for c in counts]
    streams = [long[0][b, :counts[b] + Ts - 1].tolist() for b in range(B)]
    for fb in (["perfect", "wrong_everywhere", "ngram"], ["ngram", "perfect", "wrong_everywhere"]):
        want = pair.check(rqs([drafts_for(f, streams[b]) for b, f in enumerate(fb)]), tag=f"int8 {fb}")
        assert want[1] == counts
    pair.close()


# ── 10. log-probabilities ──────────────────────────────────────────────────────────────────────────────────────────────

def test_logprobs_are_over_the_raw_row_per_sequence(hip_backend):
    """flags (1, 0, 1); sequence 0 dead-ends after six tokens: NaN behind n_produced, a NaN row for sequence 1, and the values of the
    masked sequence are those of the raw row — the reference computes them without looking at the automaton"""
    Ts = 4
    pair = Pair(hip_backend, SD.tiny(), 3, Ts)
    chain = chain_dfa(V, 7)
    for dfas, states, made in (((chain, SEEDED, None), (0, 1, 0), [6, 17, N]), ((TEMPLATE, SEEDED, None), (0, 1, 0), COUNTS)):
        rqs = three(pair, dfas=dfas, states=states)
        want = pair.check(rqs, logprobs=[True, False, True], tag="logprobs")
        assert want[1] == made
        got = pair.got(rqs, logprobs=[True, False, True])
        lp = BS.bits(got[3])
        assert lp.shape == (3, N) and np.all(lp[1] == NAN_WORD) and np.all(lp[0, made[0]:] == NAN_WORD)
        assert not np.any(lp[0, :made[0]] == NAN_WORD) and not np.any(lp[2] == NAN_WORD) and np.all(np.asarray(got[3])[0, :made[0]] <= 0)
        plain = pair.got(rqs)  # the same call without the word gives the same tokens
        assert plain[0].tolist() == got[0].tolist() and plain[2] == got[2] and plain[-1] == got[-1]
    pair.close()


# ── 11. alternation on one program ─────────────────────────────────────────────────────────────────────────────────────

def test_constrained_detached_sampled_and_greedy_calls_alternate_on_one_program(hip_backend):
    Ts = 4
    pair = Pair(hip_backend, SD.tiny(), 3, Ts)
    hists = [None, pair.prompt, None]
    con, con_pen = three(pair), three(pair, [dict(KW[0], **PEN), dict(KW[1]), dict(KW[2], **PEN)])
    free = [BCM.Request(r.first, r.start, r.n, r.sampling, history=r.history) for r in con]
    want = {"constrained": pair.want(con), "constrained_penalised": pair.want(con_pen), "sampled": pair.want(free)}
    assert want["constrained"][0].tolist() != want["sampled"][0].tolist()  # the constraint does something

    def detach():
        for b in range(3):
            pair.s.set_constraint(None, seq=b)

    calls = {
        "constrained": lambda: pair.got(con),
        "sampled": lambda: (detach(), pair.s.resident_decode_batch_speculative_sampled(FIRSTS, STARTS, COUNTS, [r.sampling for r in con], histories=hists))[1],
        "constrained_logprobs": lambda: pair.got(con, logprobs=[True, False, True]),
        "greedy": lambda: (detach(), pair.s.resident_decode_batch_speculative(FIRSTS, STARTS, COUNTS, histories=hists))[1],
        "constrained_penalised": lambda: pair.got(con_pen),
    }
    first = {}
    for rnd in range(2):
        for name, fn in calls.items():
            d0 = SD._dispatches(hip_backend, pair.s.handle)
            r = fn()
            d1 = SD._dispatches(hip_backend, pair.s.handle)
            assert not hip_backend.last_error(), hip_backend.last_error()
            plain = [x.tolist() if isinstance(x, np.ndarray) and x.dtype != np.float32 else BS.bits(x).tolist() if isinstance(x, np.ndarray) else x for x in r]
            plain.append((d1[0] - d0[0], d1[1] - d0[1]))  # every call launches what it launched before
            assert first.setdefault(name, plain) == plain, (rnd, name)
    for name in ("constrained", "constrained_penalised"):
        pair.compare(want[name], calls[name](), tag=name)
    pair.compare(want["constrained"], calls["constrained_logprobs"](), logprobs=[True, False, True], tag="constrained_logprobs")
    assert first["sampled"][0] == want["sampled"][0].tolist() and first["sampled"][2] == want["sampled"][2]
    assert first["greedy"][0] == calls["greedy"]()[0].tolist()
    pair.close()


# ── 12. refusals ───────────────────────────────────────────────────────────────────────────────────────────────────────

def raw_call(be, s, first, start, n, max_tokens, opts, sampling, out, produced=None, stats=None):
    a = [None if x is None else np.ascontiguousarray(x, dtype=np.uint32) for x in (first, start, n)]
    ptr = [None if x is None else x.ctypes.data_as(u32p) for x in a]
    return capi.load_hip().zgml_hip_resident_decode_batch_speculative_constrained(be.ctx, s.handle, ptr[0], ptr[1], ptr[2], max_tokens, opts, sampling,
                                                                                  None if out is None else out.ctypes.data, produced, stats)


def test_refusals_enqueue_nothing_and_the_next_call_works(hip_backend):
    """everything zgml_hip_resident_decode_batch_speculative_sampled refuses, with an automaton attached: nothing is enqueued, no
    state moves"""
    be, cfg, B, Ts = hip_backend, SD.tiny(), 2, 4
    hip, L = capi.load_hip(), cfg.max_seq_len
    pair = Pair(be, cfg, B, Ts, behind=())
    s = pair.s
    good = [S(**KW[0]), S(**KW[1])]
    good_c = (capi.SamplingC * B)(*good)
    pair.attach([BCM.Request(1, 0, 4, good[0], dfa=TEMPLATE, state=2), BCM.Request(1, 0, 4, good[1])])
    before = SD._dispatches(be, s.handle)

    def untouched(text):
        assert SD._dispatches(be, s.handle) == before and s.constraint_state(seq=0) == 2 and s.constraint_state(seq=1) == -1, text

    def refused(call, text):
        with pytest.raises(RuntimeError, match=text):
            call()
        hip.zgml_hip_clear_error(be.ctx)
        untouched(text)

    def raw_refused(text, handle_of, *args):
        assert raw_call(be, handle_of, *args) == -1
        assert re.search(text, be.last_error()), (text, be.last_error())
        hip.zgml_hip_clear_error(be.ctx)
        untouched(text)

    call = s.resident_decode_batch_speculative_constrained
    refused(lambda: call([1, 1], [0, 0], [4, 4], [good[0], S(temperature=0.0)]), r"sequence 1.*temperature")
    refused(lambda: call([1, 1], [0, 0], [4, 4], [S(top_p=1.5), good[1]]), r"sequence 0.*top_p")
    refused(lambda: call([1, 1], [0, 0], [4, 4], [good[0], S(stop=[V])]), r"sequence 1.*stop token")
    refused(lambda: call([1, 1], [0, 0], [4, 4], [good[0], S(recent=[1, 2], **KW[1], **PEN)]), r"sequence 1.*recent must be NULL")
    refused(lambda: call([1, 1], [0, 0], [4, 4], [S(repeat_penalty=1.2), good[1]]), r"sequence 0.*penalty_window > 0")
    refused(lambda: call([1, V], [0, 0], [4, 4], good), r"sequence 1.*token out of range")
    refused(lambda: call([1, 1], [0, 3], [4, 4], good, histories=[None, [1, 2]]), r"sequence 1.*n_history")
    refused(lambda: call([1, 1], [0, 0], [4, 4], good, ngram=5), "ngram")
    refused(lambda: call([1, 1], [0, L - Ts - 3], [4, 4], good), r"sequence 1.*max_seq")  # start + n + Ts = max_seq + 1
    refused(lambda: call([1, 1], [0, L - Ts + 1], [4, 0], good), r"sequence 1.*max_seq")  # ... of a sequence that only idles
    out = np.full(B * 4, -77, np.int64)
    raw_refused(r"sequence 0.*max_tokens", s, [1, 1], [0, 0], [5, 2], 4, None, good_c, out)
    raw_refused("no sampling parameters", s, [1, 1], [0, 0], [4, 4], 4, None, None, out)
    raw_refused("NULL", s, None, [0, 0], [4, 4], 4, None, good_c, out)
    raw_refused("NULL", s, [1, 1], None, [4, 4], 4, None, good_c, out)
    raw_refused("NULL", s, [1, 1], [0, 0], None, 4, None, good_c, out)
    raw_refused("NULL", s, [1, 1], [0, 0], [4, 4], 4, None, good_c, None)
    assert np.all(out == -77)  # a refused call writes no token either
    # all counts zero: 0, nothing touched
    toks, produced, stats = call([1, 1], [0, 0], [0, 0], good)
    assert toks.shape == (B, 0) and produced.tolist() == [0, 0] and stats == [ZERO, ZERO]
    untouched("all counts zero")
    # a batched plan with one column per sequence, and a plain plan
    s1, bm1 = batch_session(be, cfg, B, 1, like=pair.bm)
    raw_refused("one column per sequence", s1, [1, 1], [0, 0], [4, 4], 4, None, good_c, out)
    sp, mp = SD.spec_session(be, cfg, Ts)
    raw_refused("not a batched program", sp, [1, 1], [0, 0], [4, 4], 4, None, good_c, out)
    assert np.all(out == -77)
    # the two old batched speculative calls keep refusing the attached constraint, with their old message
    refused(lambda: s.resident_decode_batch_speculative_sampled([1, 1], [0, 0], [4, 4], good), "constraint is attached")
    refused(lambda: s.resident_decode_batch_speculative([1, 1], [0, 0], [4, 4]), "constraint is attached")
    # the edge that is allowed: start + n + Ts == max_seq
    toks, produced, _ = call([1, 1], [L - Ts - 4, 0], [4, L - Ts], good)
    assert produced.tolist() == [4, L - Ts] and not be.last_error(), be.last_error()
    # ... and the next valid call gives what the replay gives
    pair.check([BCM.Request(FIRST_AT_0, 0, 9, good[0], dfa=TEMPLATE, state=0), BCM.Request(FIRST_AT_8, 0, 5, good[1])], tag="after the refusals")
    for x in (s1, bm1, sp, mp):
        x.close()
    pair.close()
