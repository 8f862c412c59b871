"""CPU tests of sampled speculative decode under batching (include/zgml_hip.h: zgml_hip_resident_decode_batch_speculative_sampled).

The lock-step model tests/batch_spec_sampled_model.py runs on the oracle over a B x Ts batched plan. There the rows of the batched plan
are bit-identical to an independent token_len = Ts session of the same weights (tests/test_batch_spec_host.py
asserts it), so every sequence's stream, count and statistics must equal tests/spec_sampled_model.py's single-sequence loop run for
that sequence ALONE over such a session: tokens depend neither on the drafts nor on the batch. Checked for all draft forms, with a
stop token, with an idle sequence and with penalties. Then: the entry point is exported and mirrored."""
from pathlib import Path

import numpy as np
import pytest

from zgml_amd import capi, llama
from tests import batch_spec_sampled_model as BM
from tests import spec_sampled_model as SSM
from tests.test_penalty_host import c_sample_penalized
from tests.test_sample_host import c_sample
from tests.test_spec_sampled_host import drafts_of

ROOT = Path(__file__).resolve().parent.parent
S = capi.SamplingC.of
N, PROMPT_LEN = 24, 4
PARAMS = [dict(temperature=0.8, top_k=40, top_p=0.95, seed=1234, stream=0), dict(temperature=1.5, top_k=256, top_p=1.0, seed=77, stream=1),
          dict(temperature=1.1, top_k=64, top_p=0.9, seed=5 << 32, stream=2)]
FIRSTS, STARTS, COUNTS = [3, 90, 17], [0, PROMPT_LEN, 0], [N, 17, N]
PEN = dict(repeat_penalty=1.3, frequency_penalty=0.4, presence_penalty=0.2, penalty_window=6)


def tiny():
    return llama.preset("tiny", 64)


def prompt(cfg):
    return [(7 * i + 3) % cfg.vocab_size for i in range(PROMPT_LEN)]


class Plans:
    """The batched B x Ts plan and B independent token_len = Ts sessions on the oracle; sequence 1 sits behind the prompt in both."""

    def __init__(self, oracle, B, Ts):
        self.B, self.Ts, self.cfg = B, Ts, tiny()
        self.fns, self.ob = oracle.backend_fns(), oracle.OracleBackend()
        self.bm = llama.BatchModel(self.cfg, B, llama.Q4_0, tokens_per_seq=Ts)
        self.bs = llama.BatchSession(self.bm, self.fns, B)
        self.models = [llama.Model(self.cfg, llama.Q4_0, token_len=Ts) for _ in range(B)]
        self.sess = [llama.Session(m, self.fns) for m in self.models]
        p = prompt(self.cfg)
        for at in range(0, PROMPT_LEN, Ts):  # (the other sequences' columns run token 0 from position 0: rewritten by their own first steps)
            toks = [0] * (B * Ts)
            toks[Ts:2 * Ts] = p[at:at + Ts]
            self.bs.step(toks, [0, at] + [0] * (B - 2))
            self.sess[1].prefill(p[at:at + Ts], at, want_logits=False)

    def step(self, tokens, positions):
        return self.bs.step(tokens, positions)[1]

    def rows_of(self, b, rq):
        """rows_fn of the single-sequence loop for sequence b alone: row j sampled at pos + j with the window the contract names —
        the confirmed tokens (tracked here from the loop's own calls: the tokens between two calls' positions are the earlier
        call's accepted picks) and the candidates c[1..j]"""
        V, Ts, sp = self.cfg.vocab_size, self.Ts, rq.sampling
        at = {rq.start: rq.first}
        for q, t in enumerate(rq.history or []):
            at[q] = t
        last = []

        def rows(c, pos):
            if last:
                p0, g0 = last[0]
                for k in range(pos - p0):
                    at[p0 + 1 + k] = g0[k]
            assert at[pos] == c[0]
            self.sess[b].prefill(c, pos, want_logits=False)
            logits = self.ob.buffer(self.sess[b].handle, self.models[b].buf("logits"))[:Ts * V].reshape(Ts, V)
            confirmed = [at[q] for q in range(min(at), pos + 1)]
            if rq.penalized:
                g = [c_sample_penalized(logits[j], sp, pos + j, confirmed + [int(t) for t in c[1:j + 1]]) for j in range(Ts)]
            else:
                g = [c_sample(logits[j], sp, pos + j) for j in range(Ts)]
            last[:] = [(pos, g)]
            return g
        return rows

    def alone(self, b, rq):
        return SSM.spec_loop(self.rows_of(b, rq), rq.first, rq.start, rq.n, self.Ts, history=rq.history, drafts=rq.drafts, stop=rq.stop)

    def close(self):
        self.bs.close(), self.bm.close()
        for s, m in zip(self.sess, self.models):
            s.close(), m.close()


def requests(cfg, extra=({}, {}, {}), counts=COUNTS, drafts=(None, None, None)):
    hists = [None, prompt(cfg), None]
    return [BM.Request(FIRSTS[b], STARTS[b], counts[b], S(**PARAMS[b], **extra[b]), history=hists[b], drafts=drafts[b]) for b in range(3)]


def check_against_alone(pl, rqs):
    toks, produced, stats, _ = BM.lockstep(pl.step, pl.Ts, rqs)
    for b, rq in enumerate(rqs):
        want, n_want, st_want = pl.alone(b, rq) if rq.n else ([], 0, {"steps": 0, "drafted": 0, "accepted": 0})
        assert toks[b, :rq.n].tolist() == want and np.all(toks[b, rq.n:] == -1), b
        assert produced[b] == n_want and stats[b] == st_want, (b, stats[b], st_want)
    return toks, produced, stats


@pytest.mark.parametrize("Ts", [2, 4])
def test_every_sequence_equals_its_single_sequence_loop(oracle, Ts):
    pl = Plans(oracle, 3, Ts)
    cfg, V = pl.cfg, pl.cfg.vocab_size
    # the streams, from runs without any draft, Ts - 1 tokens longer: perfect drafts exist for the last step
    long = requests(cfg, counts=[n + Ts - 1 for n in COUNTS], drafts=([], [], []))
    ref, n_ref, _ = check_against_alone(pl, long)
    streams = [ref[b, :n_ref[b]].tolist() for b in range(3)]
    assert all(len(set(st)) > 3 for st in streams)  # precondition: it does sample
    forms = ["perfect", "ngram", "wrong_everywhere"]
    for rot in range(3):
        fb = [forms[(b + rot) % 3] for b in range(3)]
        drafts = [drafts_of(fb[b], streams[b], V) for b in range(3)]
        for b in range(3):
            if fb[b] == "wrong_everywhere":
                assert all(d != t for d, t in zip(drafts[b], streams[b]))
        toks, produced, stats = check_against_alone(pl, requests(cfg, drafts=drafts))
        for b in range(3):  # the drafts and the batch decide the steps, never the tokens
            n, steps = COUNTS[b], -(-COUNTS[b] // Ts)
            assert toks[b, :n].tolist() == streams[b][:n] and produced[b] == n, (fb, b)
            if fb[b] == "perfect":
                assert stats[b] == {"steps": steps, "drafted": steps * (Ts - 1), "accepted": steps * (Ts - 1)}
            if fb[b] == "wrong_everywhere":
                assert stats[b] == {"steps": n, "drafted": n * (Ts - 1), "accepted": 0}
    # a stop token of sequence 1 inside a step under perfect drafts, sequence 2 idle from the start
    at = next(i for i in range(Ts, 16) if streams[1][i] not in streams[1][:i] and i % Ts == (1 if Ts > 2 else 0))
    stop = [{}, dict(stop=[streams[1][at]]), {}]
    toks, produced, stats = check_against_alone(pl, requests(cfg, extra=stop, counts=[N, 17, 0], drafts=[None, streams[1], None]))
    assert produced == [N, at + 1, 0] and toks[1, :at + 1].tolist() == streams[1][:at + 1] and np.all(toks[1, at + 1:] == -1)
    assert toks[0].tolist() == streams[0][:N] and np.all(toks[2] == -1) and stats[2] == {"steps": 0, "drafted": 0, "accepted": 0}
    assert stats[1]["steps"] == at // Ts + 1
    pl.close()


@pytest.mark.parametrize("Ts", [2, 4])
def test_penalties_side_by_side(oracle, Ts):
    """penalties on for sequences 0 and 2 (sequence 1, behind the prompt, has them too in a second run: its window reaches into the
    history), off for the others: each equals its own single-sequence loop, and the penalties do something"""
    pl = Plans(oracle, 3, Ts)
    cfg = pl.cfg
    plain, _, _ = check_against_alone(pl, requests(cfg))
    for extra in ((PEN, {}, PEN), ({}, PEN, {})):
        for drafts in ((None, None, None), ([], [], [])):
            toks, produced, _ = check_against_alone(pl, requests(cfg, extra=extra, drafts=drafts))
            assert produced == COUNTS
            for b in range(3):
                assert (toks[b].tolist() != plain[b].tolist()) == bool(extra[b]), b
    pl.close()


def test_entry_point_is_exported_and_mirrored():
    if not capi.HIP_LIB_PATH.exists():
        import __graft_entry__ as g
        g.build_hip()
    lib = capi.load_hip()
    name = "zgml_hip_resident_decode_batch_speculative_sampled"
    assert name in capi.HIP_SYMBOLS and hasattr(lib, name)
    # ctx, program, first_tokens, start_pos, n_tokens, max_tokens, per_seq, sampling, tokens_out, n_produced, stats
    assert len(getattr(lib, name).argtypes) == 11
    assert name in (ROOT / "include" / "zgml_hip.h").read_text()
    assert hasattr(llama.BatchSession, "resident_decode_batch_speculative_sampled")
