"""A small Python model of sampled speculative decode under batching (the contract in include/zgml_hip.h,
zgml_hip_resident_decode_batch_speculative_sampled): B sequences of a batched plan with Ts columns each, driven in LOCK-STEP — per step
the candidates of all B sequences, ONE execution of the plan over the B * Ts tokens (step_fn), every logits row b * Ts + j sampled
by zgml_amd/csrc/sample.h through the CPU probes at its sequence's position + j with its sequence's parameters and window, then the
acceptance per sequence. The draft rules, the acceptance rule and the stop cut are tests/spec_model.py's and
tests/spec_sampled_model.py's, imported, not repeated. A sequence that has its count, or that a stop token finished, idles: it runs
its confirmed token Ts times at its end position, as the contract says, and changes nothing of its own.

tests/test_batch_spec_sampled_host.py runs it on the oracle against the single-sequence model; tests/test_hip_batch_spec_sampled.py
takes every reference from it, over the same plan stepped through the vtable. Written from the contract, with Python lists."""
import numpy as np

from tests import spec_model as SM
from tests import spec_sampled_model as SSM
from tests.test_logprob_host import c_logprob
from tests.test_penalty_host import c_sample_penalized
from tests.test_sample_host import c_sample

NAN = np.float32(np.nan)


class Request:
    """One sequence's request: first token, start position, count, its capi.SamplingC (the stop set and the penalties are read
    from it; its `recent` is not: the tokens before the call are `history`), history / drafts as in the single-sequence call."""

    def __init__(self, first, start, n, sampling, history=None, drafts=None):
        self.first, self.start, self.n, self.sampling = int(first), int(start), int(n), sampling
        self.history = None if history is None else [int(t) for t in history]
        self.drafts = None if drafts is None else [int(t) for t in drafts]

    @property
    def stop(self):
        return {int(self.sampling.stop[i]) for i in range(self.sampling.n_stop)}

    @property
    def penalized(self):
        sp = self.sampling
        neutral = sp.repeat_penalty in (0.0, 1.0) and sp.presence_penalty == 0.0 and sp.frequency_penalty == 0.0
        return not neutral and sp.penalty_window > 0


class _Seq:
    def __init__(self, rq):
        self.rq = rq
        known = rq.history or []
        self.lo = 0 if known else rq.start  # first position the history knows
        self.hist = known + [rq.first]      # the tokens at positions lo .. pos
        assert len(self.hist) == rq.start - self.lo + 1
        self.pos, self.out, self.lps, self.stopped = rq.start, [], [], False
        self.stats = {"steps": 0, "drafted": 0, "accepted": 0}

    @property
    def active(self):
        return len(self.out) < self.rq.n and not self.stopped

    def candidates(self, Ts, ngram):
        if not self.active:  # idles: the confirmed token at its end position
            return [self.hist[-1]] * Ts, 0
        if self.rq.drafts is not None:
            return SM.candidates_provided(self.hist[-1], self.pos, self.rq.start, self.rq.drafts, Ts)
        return SM.candidates_lookup(self.hist, self.pos - self.lo, Ts, ngram)

    def pick(self, row, c, j):
        """sample.h's token of candidate row j: position pos + j, window = the confirmed tokens and the candidates c[1..j]"""
        sp = self.rq.sampling
        if self.rq.penalized:
            return c_sample_penalized(row, sp, self.pos + j, self.hist + [int(t) for t in c[1:j + 1]])
        return c_sample(row, sp, self.pos + j)

    def advance(self, c, real, rows):
        g = [self.pick(rows[j], c, j) for j in range(len(c))]
        a = SM.accept(c, g)
        m, self.stopped = SSM.stop_cut(g, min(a + 1, self.rq.n - len(self.out)), self.rq.stop)
        self.out += g[:m]
        self.lps += [c_logprob(rows[k], g[k]) for k in range(m)]
        self.hist += g[:m]
        self.pos += m
        self.stats["steps"] += 1
        self.stats["drafted"] += real
        self.stats["accepted"] += a  # (before any cut)


def lockstep(step_fn, Ts, requests, ngram=2, max_tokens=None):
    """step_fn(tokens[B * Ts], positions[B]) -> logits[B * Ts, vocab]: one execution of the batched plan.
    -> (tokens[B, max_tokens] with -1 behind a count or a stop token, n_produced[B], statistics per sequence,
        float32[B, max_tokens] log-probabilities of the emitted tokens, NaN behind them)"""
    seqs = [_Seq(rq) for rq in requests]
    width = max([rq.n for rq in requests] + [0]) if max_tokens is None else max_tokens
    while any(s.active for s in seqs):
        cands = [s.candidates(Ts, ngram) for s in seqs]
        logits = step_fn([t for c, _ in cands for t in c], [s.pos for s in seqs])
        for b, s in enumerate(seqs):
            if s.active:
                s.advance(cands[b][0], cands[b][1], logits[b * Ts:(b + 1) * Ts])
    toks = np.full((len(seqs), width), -1, np.int64)
    lps = np.full((len(seqs), width), NAN, np.float32)
    for b, s in enumerate(seqs):
        toks[b, :len(s.out)] = s.out
        lps[b, :len(s.out)] = s.lps
    return toks, [len(s.out) for s in seqs], [s.stats for s in seqs], lps
