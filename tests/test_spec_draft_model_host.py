"""CPU tests of speculative decode with a draft model (include/zgml_hip.h: zgml_hip_resident_decode_speculative_model): the loop
of tests/spec_draft_model.py on the oracle, two llama.Sessions — the target's token_len = T plan, every verify step one execution
with all T rows read, and the draft's token_len = 1 plan stepped greedily, the T-th execution of a step included. Whatever the
draft is, the tokens are the target's sequential greedy stream; the statistics below are the oracle's, and the GPU tests expect
the same. Rejected drafts leave columns behind in BOTH caches: the runs show they are always overwritten before they are read.

Draft A is the target's own configuration (full acceptance); draft B a one-layer tiny with d_ff = 128, whose first five steps
reject and which then agrees."""
import numpy as np
import pytest

from zgml_amd import capi, llama
from tests import spec_model as SM
from tests.spec_draft_model import spec_draft_loop

N, T_MAX, FIRST = 24, 5, 292  # FIRST_AT_0 of tests/test_hip_spec_decode.py
GAP = 1e-3                    # the bar of tests/test_hip_spec_decode.py
# draft B on the oracle: T -> (steps, drafted, accepted)
DRAFT_B = {2: (15, 15, 10), 3: (12, 24, 14), 4: (10, 30, 15), 5: (9, 36, 16)}


def target_cfg():
    return llama.preset("tiny", 64)


def draft_b_cfg():
    cfg = llama.preset("tiny", 64)
    cfg.n_layers, cfg.d_ff = 1, 128
    return cfg


@pytest.fixture(scope="module")
def stream(oracle):
    """the target's sequential greedy decode on the oracle, with the tie condition of the GPU tests"""
    m = llama.Model(target_cfg(), llama.Q4_0)
    s = llama.Session(m, oracle.backend_fns())
    tok, out, gaps = FIRST, [], []
    for pos in range(N + T_MAX):
        tok, logits = s.step(tok, pos)
        out.append(tok)
        gaps.append(SM.top2_gap(logits))
    s.close(), m.close()
    assert min(gaps) >= GAP, min(gaps)
    return out


class Pair:
    """the two sessions on the oracle: rows() the target's verify step, draft() one greedy draft execution (its top-two gaps kept)"""

    def __init__(self, oracle, T, draft_cfg):
        self.T, self.cfg = T, target_cfg()
        self.tm = llama.Model(self.cfg, llama.Q4_0, token_len=T)
        self.ts = llama.Session(self.tm, oracle.backend_fns())
        self.dm = llama.Model(draft_cfg, llama.Q4_0)
        self.ds = llama.Session(self.dm, oracle.backend_fns())
        self.ob, self.argmax = oracle.OracleBackend(), oracle.argmax
        self.gaps = []

    def rows(self, c, pos):
        V = self.cfg.vocab_size
        self.ts.prefill(c, pos, want_logits=False)
        logits = self.ob.buffer(self.ts.handle, self.tm.buf("logits"))[:self.T * V].reshape(self.T, V)
        return [self.argmax(logits[j]) for j in range(self.T)]

    def draft(self, tok, pos):
        nxt, logits = self.ds.step(tok, pos)
        self.gaps.append(SM.top2_gap(logits))
        return nxt

    def close(self):
        for x in (self.ts, self.tm, self.ds, self.dm):
            x.close()


@pytest.mark.parametrize("T", [2, 4, 5])
def test_draft_a_is_accepted_in_full(oracle, stream, T):
    p = Pair(oracle, T, target_cfg())
    toks, produced, stats = spec_draft_loop(p.rows, p.draft, FIRST, 0, N, T)
    steps = -(-N // T)
    assert toks == stream[:N] and produced == N
    assert stats == {"steps": steps, "drafted": steps * (T - 1), "accepted": steps * (T - 1)}
    p.close()


@pytest.mark.parametrize("T", [2, 3, 4, 5])
def test_draft_b_rejects_five_steps_then_agrees(oracle, stream, T):
    p = Pair(oracle, T, draft_b_cfg())
    accepted = []
    toks, produced, stats = spec_draft_loop(p.rows, p.draft, FIRST, 0, N, T, on_step=lambda pos, c, g, a, m: accepted.append(a))
    print(T, stats, accepted, min(p.gaps))
    assert toks == stream[:N] and produced == N
    assert (stats["steps"], stats["drafted"], stats["accepted"]) == DRAFT_B[T]
    assert accepted[:5] == [0] * 5 and all(a == T - 1 for a in accepted[5:])
    # the draft's own picks are no near-ties either, at every position it visited: the GPU draft then picks the same tokens
    assert min(p.gaps) >= GAP, min(p.gaps)
    p.close()


@pytest.mark.parametrize("draft", ["a", "b"])
def test_two_calls_equal_one(oracle, stream, draft):
    T = 4
    p = Pair(oracle, T, target_cfg() if draft == "a" else draft_b_cfg())
    a, na, _ = spec_draft_loop(p.rows, p.draft, FIRST, 0, 10, T)
    b, nb, _ = spec_draft_loop(p.rows, p.draft, a[-1], 10, 14, T)  # both caches as the first call left them
    assert (na, nb) == (10, 14) and a + b == stream[:N]
    p.close()


def _fresh_draft_logits(oracle, cfg, confirmed):
    """the draft stepped over the confirmed tokens at positions 0 .. n: the logits of its last step"""
    m = llama.Model(cfg, llama.Q4_0)
    s = llama.Session(m, oracle.backend_fns())
    for pos, t in enumerate(confirmed[:-1]):
        s.step(t, pos, want_logits=False)
    logits = s.step(confirmed[-1], len(confirmed) - 1)[1]
    s.close(), m.close()
    return logits


@pytest.mark.parametrize("draft", ["a", "b"])
@pytest.mark.parametrize("T", [2, 4, 5])
def test_the_drafts_cache_keeps_up_only_with_the_t_th_execution(oracle, stream, T, draft):
    """The cache contract on the draft's side: behind the call the draft's next step equals, to the bit, that of a draft stepped
    over the confirmed tokens. The same loop WITHOUT the T-th execution leaves the column behind every fully accepted step
    unwritten; the tokens and the acceptance of this small model do not notice, the draft's logits do."""
    cfg = target_cfg() if draft == "a" else draft_b_cfg()
    p = Pair(oracle, T, cfg)
    toks, _, _ = spec_draft_loop(p.rows, p.draft, FIRST, 0, N, T)
    want = _fresh_draft_logits(oracle, cfg, [FIRST] + toks)
    assert np.array_equal(p.ds.step(toks[-1], N)[1], want)
    p.close()
    p = Pair(oracle, T, cfg)
    tok, pos, out = FIRST, 0, []
    while len(out) < N:  # (the loop of tests/spec_draft_model.py with T - 1 draft executions per step)
        c = [tok]
        for j in range(T - 1):
            c.append(p.draft(c[j], pos + j))
        g = p.rows(c, pos)
        m = min(SM.accept(c, g) + 1, N - len(out))
        out += g[:m]
        tok, pos = g[m - 1], pos + m
    assert out == toks
    assert float(np.abs(p.ds.step(out[-1], N)[1] - want).max()) > 0.1
    p.close()


def test_entry_point_is_exported_and_mirrored():
    if not capi.HIP_LIB_PATH.exists():
        import __graft_entry__ as g
        g.build_hip()
    lib = capi.load_hip()
    assert "zgml_hip_resident_decode_speculative_model" in capi.HIP_SYMBOLS and hasattr(lib, "zgml_hip_resident_decode_speculative_model")
    assert len(lib.zgml_hip_resident_decode_speculative_model.argtypes) == 12
    assert hasattr(llama.Session, "resident_decode_speculative_model")
