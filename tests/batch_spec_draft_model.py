"""A small Python model of speculative decode with a draft model under batching (the contract in include/zgml_hip.h,
zgml_hip_resident_decode_batch_speculative_model): B loops of tests/spec_draft_model.spec_draft_loop in LOCK-STEP over two batched
plans. Per step every sequence hands the draft (hist[pos], pos); the draft plan — one column per sequence — executes T times, its
greedy token of row b becoming sequence b's next candidate (the T-th execution is there for its KV column alone); ONE execution
of the target plan runs the B * T candidates; every active sequence accepts on its own rows. A sequence that has its count, or
that a stop token finished, idles: it still hands the draft (hist[pos], pos) at its end position and the draft runs on from there,
its candidates behind c[0] are whatever the draft said, and nothing of its own changes.

The acceptance rule is tests/spec_model.py's, the stop cut tests/spec_sampled_model.py's, the sampled picks and the request those
of tests/batch_spec_sampled_model.py: imported, not repeated. tests/test_batch_spec_draft_model_host.py runs it on the oracle
against the single-sequence loop; tests/test_hip_batch_spec_draft_model.py takes every reference from it."""
import numpy as np

from tests import batch_spec_sampled_model as BSM
from tests import spec_model as SM
from tests import spec_sampled_model as SSM
from tests.test_logprob_host import c_logprob

NAN = np.float32(np.nan)


class Request(BSM.Request):
    """One sequence's request; sampling=None: the greedy verify step (first maxima, no stop tokens). No drafts: the model drafts."""

    def __init__(self, first, start, n, sampling=None, history=None):
        super().__init__(first, start, n, sampling, history)

    @property
    def stop(self):
        return set() if self.sampling is None else BSM.Request.stop.fget(self)

    @property
    def penalized(self):
        return self.sampling is not None and BSM.Request.penalized.fget(self)


class _Seq(BSM._Seq):
    def pick(self, row, c, j):
        if self.rq.sampling is None:
            return int(np.argmax(row))  # the first maximum
        return super().pick(row, c, j)

    def advance(self, c, T, rows, on_step, b):
        g = [self.pick(rows[j], c, j) for j in range(T)]
        a = SM.accept(c, g)
        m, self.stopped = SSM.stop_cut(g, min(a + 1, self.rq.n - len(self.out)), self.rq.stop)
        if on_step:
            on_step(b, self.pos, list(c), g, a, m)
        self.out += g[:m]
        if self.rq.sampling is not None:
            self.lps += [c_logprob(rows[k], g[k]) for k in range(m)]
        self.hist += g[:m]
        self.pos += m
        self.stats["steps"] += 1
        self.stats["drafted"] += T - 1  # no pads
        self.stats["accepted"] += a     # (before any cut)


def lockstep(step_fn, draft_fn, T, requests, on_step=None, on_draft=None, max_tokens=None, draft_execs=None):
    """step_fn(tokens[B * T], positions[B]) -> logits[B * T, vocab]: one execution of the target's batched plan.
    draft_fn(tokens[B], positions[B]) -> logits[B, vocab]: one execution of the draft's, which stores column positions[b] of
    every sequence b. on_step(b, pos, c, g, a, m): once per step and ACTIVE sequence; on_draft(b, pos, row): every draft logits
    row of an active sequence (for the conditions a test asserts on its reference). draft_execs: executions per step when not T
    (a test's counter-example).
    -> (tokens[B, max_tokens] with -1 behind a count or a stop token, n_produced[B], statistics per sequence,
        float32[B, max_tokens] log-probabilities of the emitted tokens of the sampled sequences, NaN elsewhere)"""
    seqs = [_Seq(rq) for rq in requests]
    B = len(seqs)
    width = max([rq.n for rq in requests] + [0]) if max_tokens is None else max_tokens
    execs = T if draft_execs is None else draft_execs
    while any(s.active for s in seqs):
        cands = [[s.hist[-1]] for s in seqs]  # c[0] = hist[pos], of an idling sequence too
        for j in range(execs):
            rows = draft_fn([c[j] for c in cands], [s.pos + j for s in seqs])
            for b in range(B):
                if on_draft and seqs[b].active:
                    on_draft(b, seqs[b].pos + j, rows[b])
                if j < T - 1:
                    cands[b].append(int(np.argmax(rows[b])))
        for c in cands:  # (only the counter-example: fewer executions than candidates)
            c += [c[-1]] * (T - len(c))
        logits = step_fn([t for c in cands for t in c], [s.pos for s in seqs])
        for b, s in enumerate(seqs):
            if s.active:
                s.advance(cands[b], T, logits[b * T:(b + 1) * T], on_step, b)
    toks = np.full((B, width), -1, np.int64)
    lps = np.full((B, width), NAN, np.float32)
    for b, s in enumerate(seqs):
        toks[b, :len(s.out)] = s.out
        lps[b, :len(s.lps)] = s.lps
    return toks, [len(s.out) for s in seqs], [s.stats for s in seqs], lps
