"""CPU tests of speculative decode with a draft model under batching (include/zgml_hip.h:
zgml_hip_resident_decode_batch_speculative_model): the lock-step loop of tests/batch_spec_draft_model.py on the oracle, over two
llama.BatchSessions — the target's tokens_per_seq = T plan, every verify step one execution with all B T rows read, and the draft's
one-column plan stepped greedily, the T-th execution of a step included. On the oracle a row of a batched plan is bit-identical to
the single-sequence plan's (tests/test_batch_spec_host.py), so every sequence gets the tokens and the statistics of the
single-sequence loop of tests/test_spec_draft_model_host.py, whose constants these are, whatever the other sequences do.

Draft A is the target's own configuration (full acceptance); draft B a one-layer tiny with d_ff = 128."""
import numpy as np
import pytest

from zgml_amd import capi, llama
from tests import spec_model as SM
from tests.batch_spec_draft_model import Request, lockstep
from tests.test_spec_draft_model_host import DRAFT_B, FIRST, GAP, N, draft_b_cfg, target_cfg

B = 3
LONGEST = N + 4  # tokens of the sequence that goes furthest (the ragged calls)


@pytest.fixture(scope="module")
def stream(oracle):
    """the target's sequential greedy decode on the oracle from (FIRST, 0), with the tie condition of the GPU tests"""
    m = llama.Model(target_cfg(), llama.Q4_0)
    s = llama.Session(m, oracle.backend_fns())
    tok, out, gaps = FIRST, [], []
    for pos in range(LONGEST + 5):
        tok, logits = s.step(tok, pos)
        out.append(tok)
        gaps.append(SM.top2_gap(logits))
    s.close(), m.close()
    assert min(gaps) >= GAP, min(gaps)
    return out


class BatchPair:
    """the two batched sessions on the oracle: step() the target's verify step, draft() one draft execution of all sequences"""

    def __init__(self, oracle, T, draft_cfg):
        self.T = T
        self.tm = llama.BatchModel(target_cfg(), B, llama.Q4_0, tokens_per_seq=T)
        self.ts = llama.BatchSession(self.tm, oracle.backend_fns(), B)
        self.dm = llama.BatchModel(draft_cfg, B, llama.Q4_0)
        self.ds = llama.BatchSession(self.dm, oracle.backend_fns(), B)

    def step(self, tokens, positions):
        return self.ts.step(tokens, positions)[1]

    def draft(self, tokens, positions):
        return self.ds.step(tokens, positions)[1]

    def close(self):
        for x in (self.ts, self.tm, self.ds, self.dm):
            x.close()


def _all_from_zero(n=N):
    return [Request(FIRST, 0, n) for _ in range(B)]


@pytest.mark.parametrize("T", [2, 4, 5])
def test_draft_a_is_accepted_in_full_by_every_sequence(oracle, stream, T):
    p = BatchPair(oracle, T, target_cfg())
    toks, produced, stats, _ = lockstep(p.step, p.draft, T, _all_from_zero())
    steps = -(-N // T)
    for b in range(B):
        assert toks[b].tolist() == stream[:N] and produced[b] == N
        assert stats[b] == {"steps": steps, "drafted": steps * (T - 1), "accepted": steps * (T - 1)}
    p.close()


@pytest.mark.parametrize("T", [2, 4, 5])
def test_draft_b_gives_every_sequence_the_single_sequence_statistics(oracle, stream, T):
    p = BatchPair(oracle, T, draft_b_cfg())
    gaps = []
    toks, produced, stats, _ = lockstep(p.step, p.draft, T, _all_from_zero(), on_draft=lambda b, pos, row: gaps.append(SM.top2_gap(row)))
    for b in range(B):
        assert toks[b].tolist() == stream[:N] and produced[b] == N
        assert (stats[b]["steps"], stats[b]["drafted"], stats[b]["accepted"]) == DRAFT_B[T]
    # the draft's own picks are no near-ties, at every position a sequence visited: the GPU draft then picks the same tokens
    assert min(gaps) >= GAP, min(gaps)
    p.close()


FIRST_CALL, SECOND_CALL, THIRD_CALL = (10, 5, 24), (14, 12, 0), (0, 0, 4)


def _ragged_calls(p, T, draft_execs=None):
    """the three calls over one pair of caches -> (tokens per sequence, statistics of every call, end position per sequence)"""
    out, pos, last, all_stats = [[] for _ in range(B)], [0] * B, [FIRST] * B, []
    for counts in (FIRST_CALL, SECOND_CALL, THIRD_CALL):
        rq = [Request(last[b], pos[b], counts[b], history=[FIRST] + out[b][:-1] if pos[b] else None) for b in range(B)]
        toks, produced, stats, _ = lockstep(p.step, p.draft, T, rq, draft_execs=draft_execs)
        assert tuple(produced) == counts
        for b in range(B):
            out[b] += toks[b, :counts[b]].tolist()
            pos[b] += counts[b]
            last[b] = out[b][-1] if out[b] else FIRST
        all_stats.append(stats)
    return out, all_stats, pos


@pytest.mark.parametrize("draft", ["a", "b"])
def test_ragged_calls_give_the_streams_of_one_call(oracle, stream, draft):
    T = 4
    p = BatchPair(oracle, T, target_cfg() if draft == "a" else draft_b_cfg())
    out, stats, pos = _ragged_calls(p, T)
    assert pos == [24, 17, 28]
    for b in range(B):
        assert out[b] == stream[:pos[b]], b
    assert stats[1][2] == {"steps": 0, "drafted": 0, "accepted": 0}  # the sequence that idled through the second call
    assert stats[2][0] == stats[2][1] == {"steps": 0, "drafted": 0, "accepted": 0}
    assert stats[2][2]["steps"] >= 1
    p.close()


def _fresh_draft_logits(oracle, cfg, confirmed):
    """a single-sequence draft stepped over the confirmed tokens at positions 0 .. n: the logits of its last step"""
    m = llama.Model(cfg, llama.Q4_0)
    s = llama.Session(m, oracle.backend_fns())
    for pos, t in enumerate(confirmed[:-1]):
        s.step(t, pos, want_logits=False)
    logits = s.step(confirmed[-1], len(confirmed) - 1)[1]
    s.close(), m.close()
    return logits


@pytest.mark.parametrize("draft", ["a", "b"])
@pytest.mark.parametrize("T", [2, 4, 5])
def test_the_drafts_cache_keeps_up_per_sequence(oracle, stream, T, draft):
    """Behind the calls one step of the draft session on every sequence's confirmed token equals, to the bit, that of a fresh
    draft stepped over the sequence's confirmed tokens — for the sequence that idled through a call too. The same loop with T - 1
    executions per step leaves the column behind every fully accepted step unwritten: the draft's logits notice."""
    cfg = target_cfg() if draft == "a" else draft_b_cfg()
    p = BatchPair(oracle, T, cfg)
    out, _, pos = _ragged_calls(p, T)
    want = [_fresh_draft_logits(oracle, cfg, [FIRST] + out[b]) for b in range(B)]
    got = p.draft([out[b][-1] for b in range(B)], pos)
    for b in range(B):
        assert np.array_equal(got[b], want[b]), b
    p.close()
    p = BatchPair(oracle, T, cfg)
    out2, _, pos2 = _ragged_calls(p, T, draft_execs=T - 1)
    assert out2 == out and pos2 == pos
    got = p.draft([out[b][-1] for b in range(B)], pos)
    assert max(float(np.abs(got[b] - want[b]).max()) for b in range(B)) > 0.1
    p.close()


def test_entry_point_is_exported_and_mirrored():
    if not capi.HIP_LIB_PATH.exists():
        import __graft_entry__ as g
        g.build_hip()
    lib = capi.load_hip()
    name = "zgml_hip_resident_decode_batch_speculative_model"
    assert name in capi.HIP_SYMBOLS and hasattr(lib, name)
    assert len(getattr(lib, name).argtypes) == 13
    assert hasattr(llama.BatchSession, "resident_decode_batch_speculative_model")
