"""A small Python model of constrained speculative decode under batching (the contract in include/zgml_hip.h,
zgml_hip_resident_decode_batch_speculative_constrained): tests/batch_spec_sampled_model.py's lock-step loop with an automaton and a
state per request. Nothing is restated: the pass over a step's candidates, the state's step, forced[], the dead row and the row
without a pick are tests/spec_constraint_model.py's (constrain, step_state, forced, DEAD, NO_PICK), the draft rules, the acceptance
rule and the stop cut tests/spec_model.py's and tests/spec_sampled_model.py's, the idling and the unattached sequence's whole path
tests/batch_spec_sampled_model.py's. New here is only WHERE they apply: per sequence, each with its own automaton — or none: such a
request takes the sampled path, its rows are FREE (zgml_amd/csrc/spec.h: kSpecRowFree), its candidates untouched, `drafted` the
mode's real drafts alone.

The floating-point pick is not restated either: a constrained row's token is tests/cpp/constraint_probe.cpp's c_constraint_sample
under the row's state. tests/test_batch_spec_constraint_host.py holds this file to the single-sequence models;
tests/test_hip_batch_spec_constraint.py takes every reference from it. Written from the contract, with Python lists."""
import numpy as np

from tests import batch_spec_sampled_model as BM
from tests import spec_model as SM
from tests import spec_sampled_model as SSM
from tests.spec_constraint_model import DEAD, NO_PICK, constrain, forced, step_state
from tests.test_constraint_host import c_constraint_sample
from tests.test_logprob_host import c_logprob

FREE = 0xFFFFFFFE  # the state word of a row of a sequence without an automaton: no state of any automaton, and not DEAD


def free_rows(T):
    """the rows of an unattached sequence's step -> (row_state, forced tokens placed)"""
    return [FREE] * T, 0


def row_selects(row_state):
    """has the row candidates at all? (a dead row has none; a free row has the sampled form's, a live one its state's)"""
    return row_state != DEAD


class Request(BM.Request):
    """BM.Request with the automaton attached to the sequence (a tests.test_constraint_host.Dfa; None: nothing attached) and the
    state it stands in when the call begins"""

    def __init__(self, first, start, n, sampling, history=None, drafts=None, dfa=None, state=0):
        BM.Request.__init__(self, first, start, n, sampling, history=history, drafts=drafts)
        self.dfa, self.state = dfa, int(state)


class _Seq(BM._Seq):
    def __init__(self, rq):
        BM._Seq.__init__(self, rq)
        self.dfa = getattr(rq, "dfa", None)
        self.state = rq.state if self.dfa is not None else -1  # (-1: what zgml_hip_program_constraint_state says of a sequence without one)
        self.frc = forced(self.dfa.class_of, self.dfa.next) if self.dfa is not None else None
        self.dead_end = False
        self.seen = {}  # position -> (row state, pick) of the row that emitted the token behind it (the tests' preconditions)

    def candidates(self, Ts, ngram):
        """-> (c, what `drafted` grows by, row_state)"""
        c, real = BM._Seq.candidates(self, Ts, ngram)
        if not self.active:
            return c, 0, [DEAD] * Ts  # (no row of an idle step is picked)
        if self.dfa is None:
            row_state, placed = free_rows(Ts)
            return c, real + placed, row_state
        c, row_state, placed = constrain(c, real, self.state, self.dfa.class_of, self.dfa.next, self.frc)
        return c, real + placed, row_state

    def advance(self, c, drafted, row_state, rows):
        if self.dfa is None:  # the sampled path, whole
            assert all(s == FREE for s in row_state)
            return BM._Seq.advance(self, c, drafted, rows)
        g = []
        for j in range(len(c)):
            tok = -1
            if row_selects(row_state[j]):
                tok, _ = c_constraint_sample(rows[j], self.rq.sampling, self.pos + j, self.hist + [int(t) for t in c[1:j + 1]], self.dfa, row_state[j])
            g.append(tok if tok >= 0 else NO_PICK)
        a = SM.accept(c, g)
        m = min(a + 1, self.rq.n - len(self.out))
        if g[a] == NO_PICK:  # the reached state allows no token: cut in front of it, the sequence is finished
            m, self.dead_end = min(m, a), True
        m, stopped = SSM.stop_cut(g, m, self.rq.stop)
        self.stopped = stopped or self.dead_end  # (either way it idles from here on)
        for k in range(m):
            self.seen[self.pos + k] = (row_state[k], g[k])
            self.state = step_state(self.dfa.class_of, self.dfa.next, self.state, g[k])
            assert self.state != DEAD
        self.out += g[:m]
        self.lps += [c_logprob(rows[k], g[k]) for k in range(m)]  # (over the raw row)
        self.hist += g[:m]
        self.pos += m
        self.stats["steps"] += 1
        self.stats["drafted"] += drafted
        self.stats["accepted"] += a  # (before any cut)


def lockstep(step_fn, Ts, requests, ngram=2, max_tokens=None, seqs_out=None):
    """BM.lockstep over Requests with automata -> its four results and the sequences' states afterwards (-1: none attached).
    seqs_out: a list that receives the model's sequences (dead_end, seen) for a test's preconditions"""
    seqs = [_Seq(rq) for rq in requests]
    width = max([rq.n for rq in requests] + [0]) if max_tokens is None else max_tokens
    while any(s.active for s in seqs):
        cands = [s.candidates(Ts, ngram) for s in seqs]
        logits = step_fn([t for c, _, _ in cands for t in c], [s.pos for s in seqs])
        for b, s in enumerate(seqs):
            if s.active:
                s.advance(cands[b][0], cands[b][1], cands[b][2], logits[b * Ts:(b + 1) * Ts])
    toks = np.full((len(seqs), width), -1, np.int64)
    lps = np.full((len(seqs), width), BM.NAN, np.float32)
    for b, s in enumerate(seqs):
        toks[b, :len(s.out)] = s.out
        lps[b, :len(s.out)] = s.lps
    if seqs_out is not None:
        seqs_out[:] = seqs
    return toks, [len(s.out) for s in seqs], [s.stats for s in seqs], lps, [s.state for s in seqs]
