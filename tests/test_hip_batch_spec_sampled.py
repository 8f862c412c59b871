"""Sampled speculative decode under batching on the MI355X (zgml_hip_resident_decode_batch_speculative_sampled): B sequences on a batched
plan with Ts columns per sequence, every one running the sampled verify loop of zgml_hip_resident_decode_speculative_sampled on the
device with its own parameter set, stream, seed, stop set, penalties and `logprobs` word.

THE REFERENCE everywhere is the SAME batched plan driven from the host in lock-step with the device loop
(tests/batch_spec_sampled_model.py): per step the candidates of all B sequences, ONE BatchSession.step over the B * Ts tokens through
the vtable, all rows downloaded, row b * Ts + j sampled on the CPU by zgml_amd/csrc/sample.h (the probes c_sample /
c_sample_penalized with window = confirmed tokens + c[1..j], c_logprob for the values), the acceptance per sequence. Same kernels,
same inputs, same step grouping: bit-exact equality of tokens, counts, statistics and log-probability bits, no tolerance. A decode
plan or a differently grouped run is no reference here (a pick may turn on the last bit of the logits when the
grouping differs): always the same requests are replayed.

Every reference is computed from the reference alone; its preconditions — it does sample, "wrong" drafts are wrong everywhere, the
stream is long enough for the last step's drafts — are asserted on it before the device is asked."""
import ctypes as C
import re

import numpy as np
import pytest

from zgml_amd import capi, llama
from tests import batch_spec_sampled_model as BM
from tests import test_hip_spec_decode as SD
from tests.test_hip_batch_spec_decode import admit_prompt, batch_session, closed_form
from tests.test_hip_l7dims import l7cfg
from tests.test_hip_sample import PARAMS

pytestmark = pytest.mark.gpu

S = capi.SamplingC.of
N, PROMPT_LEN = SD.N, SD.PROMPT_LEN
FIRST_AT_0, FIRST_AT_8 = SD.FIRST_AT_0, SD.FIRST_AT_8
u32p = C.POINTER(C.c_uint32)
NAN_WORD = 0x7FC00000
ZERO = {"steps": 0, "drafted": 0, "accepted": 0}
FIRSTS, STARTS, COUNTS = [FIRST_AT_0, FIRST_AT_8, FIRST_AT_0], [0, PROMPT_LEN, 0], [N, 17, N]
# one parameter set per sequence, with its own seed and stream
KW = [dict(seed=1234, stream=0, **PARAMS["k40_p95"]), dict(seed=77, stream=3, **PARAMS["k256_p1"]), dict(seed=9 << 32, stream=1, **PARAMS["k1"])]
PEN = dict(repeat_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.4, penalty_window=16)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


class Pair:
    """The device side and the reference side of one batched plan: two sessions over the same model, sequence `behind` of both behind
    the admitted 8-token prompt. `want` replays requests on the reference session in lock-step, `got` asks the device loop."""

    def __init__(self, be, cfg, B, Ts, kvq=0, like=None, behind=(1,), threads=8):
        self.be, self.cfg, self.B, self.Ts = be, cfg, B, Ts
        self.s, self.bm = batch_session(be, cfg, B, Ts, kvq=kvq, like=like, threads=threads)
        self.host = llama.BatchSession(self.bm, llama.hip_backend_fns(be), B)
        self.prompt = None
        for seq in behind:
            self.prompt = admit_prompt(be, self.s, self.bm, seq, Ts)
            admit_prompt(be, self.host, self.bm, seq, Ts)

    def want(self, rqs, max_tokens=None):
        return BM.lockstep(lambda toks, pos: self.host.step(toks, pos)[1], self.Ts, rqs, max_tokens=max_tokens)

    def got(self, rqs, logprobs=None):
        out = self.s.resident_decode_batch_speculative_sampled([r.first for r in rqs], [r.start for r in rqs], [r.n for r in rqs], [r.sampling for r in rqs],
                                                               histories=[r.history for r in rqs], drafts=[r.drafts for r in rqs], logprobs=logprobs)
        assert not self.be.last_error(), self.be.last_error()
        return out

    def check(self, rqs, logprobs=None, tag=""):
        """the device equals the replay of the same requests -> the reference"""
        want = self.want(rqs)
        got = self.got(rqs, logprobs)
        print(tag, "produced", want[1], "stats", got[2])
        assert got[0].tolist() == want[0].tolist(), tag
        assert np.asarray(got[1]).tolist() == want[1] and got[2] == want[2], (tag, got[1], want[1], got[2], want[2])
        if logprobs is not None:
            flags = [bool(logprobs)] * self.B if isinstance(logprobs, bool) else list(logprobs)
            for b in range(self.B):
                row = bits(want[3][b]) if flags[b] else np.full(want[3].shape[1], NAN_WORD, np.uint32)
                print(tag, "sequence", b, "log-probability bits differing:", int(np.sum(bits(got[3][b]) != row)))
                assert bits(got[3][b]).tolist() == row.tolist(), (tag, b)
        return want

    def close(self):
        self.host.close(), self.s.close(), self.bm.close()


def three(pair, kw=KW, counts=COUNTS, drafts=(None, None, None), hists=None):
    hists = [None, pair.prompt, None] if hists is None else hists
    return [BM.Request(FIRSTS[b], STARTS[b], counts[b], S(**kw[b]), history=hists[b], drafts=drafts[b]) for b in range(3)]


def streams_of(pair, kw=KW, hists=None):
    """every sequence's stream from a replay without any draft, Ts - 1 tokens longer than its count: perfect drafts exist for the
    last step"""
    long = [n + pair.Ts - 1 for n in COUNTS]
    toks, produced, _, _ = pair.want(three(pair, kw, counts=long, drafts=([], [], []), hists=hists))
    assert produced == long
    return [toks[b, :long[b]].tolist() for b in range(3)]


# ── 1. tokens and statistics ───────────────────────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("Ts", [2, 4, 5])
def test_tokens_and_stats_of_three_sequences(hip_backend, Ts):
    """B = 3 (M = 6, 12, 15), counts (24, 17, 24), sequence 1 behind the admitted prompt with the prompt as history; parameter sets
    k40_p95 / k256_p1 / k1; perfect, n-gram and wrong-everywhere drafts rotate over the sequences"""
    pair = Pair(hip_backend, SD.tiny(), 3, Ts)
    V = pair.cfg.vocab_size
    streams = streams_of(pair)
    assert len(set(streams[0])) > 3 and len(set(streams[1])) > 3  # precondition: the sampled streams do sample
    forms, one_stream = ["perfect", "ngram", "wrong_everywhere"], True
    for rot in range(3):
        fb = [forms[(b + rot) % 3] for b in range(3)]
        drafts = [SD.drafts_of(fb[b], streams[b], V) for b in range(3)]
        for b in range(3):
            if fb[b] == "wrong_everywhere":
                assert all(d != t for d, t in zip(drafts[b], streams[b]))  # precondition
        want = pair.check(three(pair, drafts=drafts), tag=f"Ts {Ts} {fb}")
        for b in range(3):
            assert want[1][b] == COUNTS[b] and np.all(want[0][b, COUNTS[b]:] == -1)
            if closed_form(fb[b], COUNTS[b], Ts):
                assert want[2][b] == closed_form(fb[b], COUNTS[b], Ts), (fb, b)
            one_stream = one_stream and want[0][b, :COUNTS[b]].tolist() == streams[b][:COUNTS[b]]
    print(f"Ts {Ts}: the three draft forms gave one stream per sequence: {one_stream}")
    pair.close()


# ── 2. top_k = 1 is the greedy batched call ────────────────────────────────────────────────────────────────────────────

def test_top_k_1_equals_the_greedy_batched_call_on_the_same_session(hip_backend):
    be, Ts = hip_backend, 4
    pair = Pair(be, SD.tiny(), 3, Ts)
    V, hists = pair.cfg.vocab_size, [None, pair.prompt, None]
    kw = [dict(seed=b + 1, stream=b, **PARAMS["k1"]) for b in range(3)]
    long = [n + Ts - 1 for n in COUNTS]
    stream, _ = pair.s.resident_decode_batch_speculative(FIRSTS, STARTS, long, histories=hists)
    forms = ["perfect", "ngram", "wrong_everywhere"]
    for rot in range(3):
        drafts = [SD.drafts_of(forms[(b + rot) % 3], stream[b, :long[b]].tolist(), V) for b in range(3)]
        g_toks, g_stats = pair.s.resident_decode_batch_speculative(FIRSTS, STARTS, COUNTS, histories=hists, drafts=drafts)
        toks, produced, stats = pair.got(three(pair, kw, drafts=drafts))
        assert not be.last_error(), be.last_error()
        assert toks.tolist() == g_toks.tolist() and produced.tolist() == COUNTS and stats == g_stats, rot
    pair.close()


# ── 3. stop tokens ─────────────────────────────────────────────────────────────────────────────────────────────────────

def stop_case(pair, b, lo=4, hi=16):
    """-> (parameter sets with sequence b's stop token set, perfect drafts for b, the index of the stop): the token is taken from
    b's reference stream at an index inside a step under perfect drafts, where it occurs for the first time"""
    Ts = pair.Ts
    for seed in range(16):
        kw = [dict(k) for k in KW]
        kw[b]["seed"] = 100 + seed
        stream = streams_of(pair, kw)[b]
        at = next((i for i in range(lo, hi) if 0 < i % Ts < Ts - 1 and stream[i] not in stream[:i]), None)
        if at is not None:
            break
    else:
        pytest.fail("no reference stream emits a new token inside a step")
    assert stream.index(stream[at]) == at  # its first occurrence
    kw[b]["stop"] = [stream[at]]
    return kw, stream, at


def test_stop_token_ends_its_sequence_and_the_others_go_on(hip_backend):
    Ts = 4
    pair = Pair(hip_backend, SD.tiny(), 3, Ts)
    kw, stream, at = stop_case(pair, 1)
    drafts = [None, stream, None]
    want = pair.check(three(pair, kw, drafts=drafts), tag="stop")
    made = at + 1
    assert want[1] == [N, made, N]  # sequence 1 ends at its stop token, inside a step; the others finish
    assert want[0][1, :made].tolist() == stream[:made] and np.all(want[0][1, made:] == -1)
    assert want[2][1]["steps"] == at // Ts + 1 and want[2][1]["accepted"] == want[2][1]["steps"] * (Ts - 1)  # (accepted counts before the cut)
    # a second call continues sequence 1 while the others want nothing: the replay of those same two calls
    t0 = want[0]
    firsts2 = [int(t0[0, N - 1]), int(t0[1, made - 1]), int(t0[2, N - 1])]
    starts2 = [N, PROMPT_LEN + made, N]
    hist1 = pair.prompt + [FIRST_AT_8] + t0[1, :made - 1].tolist()
    kw2 = [dict(k) for k in kw]
    kw2[1]["stop"] = []
    rq2 = [BM.Request(firsts2[b], starts2[b], [0, 10, 0][b], S(**kw2[b]), history=[None, hist1, None][b], drafts=[None, stream[made:], None][b]) for b in range(3)]
    want2 = pair.check(rq2, tag="continued")
    assert want2[1] == [0, 10, 0] and want2[0].shape == (3, 10)
    assert np.all(want2[0][0] == -1) and np.all(want2[0][2] == -1) and want2[2][0] == ZERO and want2[2][2] == ZERO
    print("the continuation is the stream's:", want2[0][1].tolist() == stream[made:made + 10])
    pair.close()


# ── 4. penalties side by side ──────────────────────────────────────────────────────────────────────────────────────────

def test_penalties_side_by_side(hip_backend):
    """penalties on for sequences 0 and 2, off for sequence 1; sequence 2 sits behind the prompt too and its window reaches into the
    history handed over — which ends with the first two tokens of its stream without a history, so that it matters"""
    Ts = 4
    pair = Pair(hip_backend, SD.tiny(), 3, Ts, behind=(1, 2))
    p = pair.prompt
    firsts, starts = [FIRST_AT_0, FIRST_AT_8, FIRST_AT_8], [0, PROMPT_LEN, PROMPT_LEN]
    kw = [dict(KW[0], **PEN), dict(KW[1]), dict(KW[1], seed=4321, stream=5, **PEN)]
    plain_kw = [dict(KW[0]), dict(KW[1]), dict(KW[1], seed=4321, stream=5)]

    def rqs(kws, hist2, drafts=(None, None, None)):
        return [BM.Request(firsts[b], starts[b], COUNTS[b], S(**kws[b]), history=[None, p, hist2][b], drafts=drafts[b]) for b in range(3)]

    without = pair.want(rqs(kw, None))[0]
    hist2 = p[:PROMPT_LEN - 2] + without[2, :2].tolist()
    plain = pair.want(rqs(plain_kw, hist2))[0]
    for drafts in ((None, None, None), ([], [], [])):
        want = pair.check(rqs(kw, hist2, drafts), tag=f"penalised, drafts {drafts[0]}")
        assert want[1] == COUNTS
        # preconditions: the penalties do something where they are on, nothing where they are off; the history does something
        assert want[0][0].tolist() != plain[0].tolist() and want[0][2].tolist() != plain[2].tolist()
        assert want[0][1].tolist() == plain[1].tolist()
        assert want[0][2].tolist() != without[2].tolist()
    pair.close()


# ── 5. log-probabilities ───────────────────────────────────────────────────────────────────────────────────────────────

def test_logprobs_per_sequence(hip_backend):
    """flags (1, 0, 1): values bit-equal to the reference, a NaN row for sequence 1, NaN behind every count and behind a stop"""
    Ts = 4
    pair = Pair(hip_backend, SD.tiny(), 3, Ts)
    kw, stream, at = stop_case(pair, 0)
    counts = [N, N, 17]
    rq = [BM.Request(FIRSTS[b], STARTS[b], counts[b], S(**kw[b]), history=[None, pair.prompt, None][b], drafts=[stream, None, []][b]) for b in range(3)]
    want = pair.check(rq, logprobs=[True, False, True], tag="logprobs")
    assert want[1] == [at + 1, N, 17]
    got = pair.got(rq, logprobs=[True, False, True])
    lp = bits(got[3])
    assert lp.shape == (3, N) and np.all(lp[1] == NAN_WORD)
    assert np.all(lp[0, at + 1:] == NAN_WORD) and np.all(lp[2, 17:] == NAN_WORD)  # behind the stop, behind the count
    assert not np.any(lp[0, :at + 1] == NAN_WORD) and not np.any(lp[2, :17] == NAN_WORD)
    assert np.all(np.asarray(got[3])[0, :at + 1] <= 0)
    # the same call without the word gives the same tokens, and all flags off give an all-NaN table
    plain = pair.got(rq)
    assert plain[0].tolist() == got[0].tolist() and plain[2] == got[2]
    off = pair.got(rq, logprobs=False)
    assert np.all(bits(off[3]) == NAN_WORD) and off[0].tolist() == got[0].tolist()
    pair.close()


# ── 6. more than one slice and block per row ───────────────────────────────────────────────────────────────────────────

def test_three_slices_and_two_logprob_blocks_per_row(hip_backend):
    """tiny with vocab_size = 4608: 3 select slices of 1792 logits and 2 log-probability blocks of 4096, the last one short —
    the smallest shape at which the (row, slice) and (row, block) indexing of B * Ts rows can go wrong. B = 2, Ts = 3"""
    cfg = SD.tiny()
    cfg.vocab_size = 4608
    B, Ts, n = 2, 3, 13
    pair = Pair(hip_backend, cfg, B, Ts, behind=())
    kw = [dict(seed=11, stream=0, **PARAMS["k40_p95"]), dict(seed=12, stream=1, **PARAMS["k256_p1"])]
    firsts = [292, 4000]
    long = pair.want([BM.Request(firsts[b], 0, n + Ts - 1, S(**kw[b]), drafts=[]) for b in range(B)])[0]
    assert all(len(set(long[b].tolist())) > 3 for b in range(B))
    print("a token of the second log-probability block is emitted:", bool(long.max() >= 4096))  # (every block enters every value's sum anyway)
    for drafts in ([None, None], [long[0].tolist(), []], [[], long[1].tolist()]):
        rq = [BM.Request(firsts[b], 0, n, S(**kw[b]), drafts=drafts[b]) for b in range(B)]
        pair.check(rq, logprobs=True, tag=f"vocab 4608, drafts {[d if d is None else len(d) for d in drafts]}")
    pair.close()


def test_l7_dimensions_device_loop_equals_the_lockstep_replay(hip_backend):
    """Two layers at Llama-2-7B dimensions, B = 2, Ts = 4, 12 tokens: vocab 32000 is 18 slices per row. n-gram drafts, and provided
    drafts right and wrong at two places"""
    B, Ts, n = 2, 4, 12
    base = llama.Model(l7cfg(2), llama.Q4_0, threads=16)
    pair = Pair(hip_backend, base.cfg, B, Ts, like=base, behind=(), threads=16)
    V = base.cfg.vocab_size
    firsts = [20000, 4321]
    kw = [dict(temperature=1.0, top_k=40, top_p=0.9, seed=31, stream=4), dict(temperature=1.3, top_k=256, top_p=1.0, seed=32, stream=5)]
    ref = pair.want([BM.Request(firsts[b], 0, n, S(**kw[b])) for b in range(B)])[0]
    right = [ref[b].tolist() + ref[b, -1:].tolist() * Ts for b in range(B)]
    wrong = [[(t + 1) % V if i in (2, 7) else t for i, t in enumerate(r)] for r in right]
    for drafts in ([None, None], right, [wrong[0], None], [right[0], wrong[1]]):
        rq = [BM.Request(firsts[b], 0, n, S(**kw[b]), drafts=drafts[b]) for b in range(B)]
        pair.check(rq, logprobs=[False, True], tag="l7")
    pair.close(), base.close()


# ── 7. int8 KV ─────────────────────────────────────────────────────────────────────────────────────────────────────────

def test_int8_kv(hip_backend):
    B, Ts = 2, 4
    pair = Pair(hip_backend, SD.tiny(), B, Ts, kvq=32, behind=())
    kw = KW[:2]
    firsts, counts = [SD.FIRST_INT8, FIRST_AT_0], [N, 17]
    long = pair.want([BM.Request(firsts[b], 0, counts[b] + Ts - 1, S(**kw[b]), drafts=[]) for b in range(B)])[0]
    assert all(len(set(long[b, :counts[b]].tolist())) > 3 for b in range(B))
    streams = [long[b, :counts[b] + Ts - 1].tolist() for b in range(B)]
    for fb in (["perfect", "wrong_everywhere"], ["ngram", "perfect"]):
        drafts = [SD.drafts_of(f, streams[b], pair.cfg.vocab_size) for b, f in enumerate(fb)]
        want = pair.check([BM.Request(firsts[b], 0, counts[b], S(**kw[b]), drafts=drafts[b]) for b in range(B)], tag=f"int8 {fb}")
        for b in range(B):
            if closed_form(fb[b], counts[b], Ts):
                assert want[2][b] == closed_form(fb[b], counts[b], Ts), (fb, b)
    pair.close()


# ── 8. refusals ────────────────────────────────────────────────────────────────────────────────────────────────────────

def raw_call(be, s, first, start, n, max_tokens, opts, sampling, out, produced=None, stats=None):
    a = [None if x is None else np.ascontiguousarray(x, dtype=np.uint32) for x in (first, start, n)]
    ptr = [None if x is None else x.ctypes.data_as(u32p) for x in a]
    return capi.load_hip().zgml_hip_resident_decode_batch_speculative_sampled(be.ctx, s.handle, ptr[0], ptr[1], ptr[2], max_tokens, opts, sampling,
                                                                              None if out is None else out.ctypes.data, produced, stats)


def test_refusals_enqueue_nothing_and_leave_the_program_usable(hip_backend):
    be, cfg, B, Ts = hip_backend, SD.tiny(), 2, 4
    hip, V, L = capi.load_hip(), cfg.vocab_size, cfg.max_seq_len
    pair = Pair(be, cfg, B, Ts, behind=())
    s = pair.s
    good = [S(**KW[0]), S(**KW[1])]
    good_c = (capi.SamplingC * B)(*good)
    before = SD._dispatches(be, s.handle)

    def refused(call, text):
        with pytest.raises(RuntimeError, match=text):
            call()
        hip.zgml_hip_clear_error(be.ctx)
        assert SD._dispatches(be, s.handle) == before, text

    def raw_refused(text, handle_of, *args):
        assert raw_call(be, handle_of, *args) == -1
        assert re.search(text, be.last_error()), (text, be.last_error())
        hip.zgml_hip_clear_error(be.ctx)
        assert SD._dispatches(be, s.handle) == before, text

    call = s.resident_decode_batch_speculative_sampled
    # per sequence what the sampling parameters are refused for: the message names the sequence
    refused(lambda: call([1, 1], [0, 0], [4, 4], [good[0], S(temperature=0.0)]), r"sequence 1.*temperature")
    refused(lambda: call([1, 1], [0, 0], [4, 4], [S(top_p=1.5), good[1]]), r"sequence 0.*top_p")
    refused(lambda: call([1, 1], [0, 0], [4, 4], [good[0], S(stop=[V])]), r"sequence 1.*stop token")
    refused(lambda: call([1, 1], [0, 0], [4, 4], [good[0], S(recent=[1, 2], **KW[1], **PEN)]), r"sequence 1.*recent must be NULL")
    refused(lambda: call([1, 1], [0, 0], [4, 4], [S(repeat_penalty=1.2), good[1]]), r"sequence 0.*penalty_window > 0")
    # what the greedy batched call refuses: tokens, histories, the + Ts bound
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
    # a constraint attached to any sequence
    con = be.constraint_create(np.zeros(V, np.uint16), np.zeros((1, 1), np.uint16))
    s.set_constraint(con, 0, seq=1)
    refused(lambda: call([1, 1], [0, 0], [4, 4], good), "constraint is attached")
    s.set_constraint(None, seq=1)
    be.constraint_free(con)
    # all counts zero: 0, nothing touched
    toks, produced, stats = call([1, 1], [0, 0], [0, 0], good)
    assert toks.shape == (B, 0) and produced.tolist() == [0, 0] and stats == [ZERO, ZERO] and SD._dispatches(be, s.handle) == before
    # a batched plan with one column per sequence, and a plain plan
    s1, bm1 = batch_session(be, cfg, B, 1, like=pair.bm)
    raw_refused("one column per sequence", s1, [1, 1], [0, 0], [4, 4], 4, None, good_c, out)
    sp, mp = SD.spec_session(be, cfg, Ts)
    raw_refused("not a batched program", sp, [1, 1], [0, 0], [4, 4], 4, None, good_c, out)
    # zgml_hip_resident_decode_batch_sampled still refuses the Ts >= 2 plan
    prod, two = np.zeros(B, np.uint32), np.ones(B, np.uint32)
    assert hip.zgml_hip_resident_decode_batch_sampled(be.ctx, s.handle, two.ctypes.data_as(u32p), two.ctypes.data_as(u32p), two.ctypes.data_as(u32p), 2, good_c,
                                                      out.ctypes.data, prod.ctypes.data_as(u32p)) == -1
    assert "columns per sequence" in be.last_error() and SD._dispatches(be, s.handle) == before
    hip.zgml_hip_clear_error(be.ctx)
    assert np.all(out == -77)
    # the edge that is allowed: start + n + Ts == max_seq
    toks, produced, _ = call([1, 1], [L - Ts - 4, 0], [4, L - Ts], [S(**KW[0]), S(**KW[1])])
    assert toks.shape == (B, L - Ts) and produced.tolist() == [4, L - Ts] and np.all(toks[0, :4] >= 0) and np.all(toks[1] >= 0) and not be.last_error(), be.last_error()
    # ... and the program is usable: a valid call gives what the replay gives, and the vtable still steps like a fresh session's
    pair.check([BM.Request(FIRST_AT_0, 0, 9, good[0]), BM.Request(FIRST_AT_8, 0, 5, good[1])], tag="after the refusals")
    fresh = llama.BatchSession(pair.bm, llama.hip_backend_fns(be), B)
    toks8, pos = [(5 * i + 2) % V for i in range(B * Ts)], [0, 0]  # (from position 0: no column of an earlier call is read)
    n_a, l_a = s.step(toks8, pos)
    n_b, l_b = fresh.step(toks8, pos)
    assert n_a.tolist() == n_b.tolist() and np.array_equal(l_a, l_b) and not be.last_error(), be.last_error()
    for x in (fresh, s1, bm1, sp, mp):
        x.close()
    pair.close()


# ── 9. alternation on one program ──────────────────────────────────────────────────────────────────────────────────────

def test_greedy_sampled_penalised_and_logprob_calls_alternate_on_one_program(hip_backend):
    Ts = 4
    pair = Pair(hip_backend, SD.tiny(), 3, Ts)
    hists = [None, pair.prompt, None]
    pen_kw = [dict(KW[0], **PEN), dict(KW[1]), dict(KW[2], **PEN)]
    calls = {
        "greedy": lambda: pair.s.resident_decode_batch_speculative(FIRSTS, STARTS, COUNTS, histories=hists),
        "sampled": lambda: pair.got(three(pair)),
        "penalised": lambda: pair.got(three(pair, pen_kw)),
        "logprobs": lambda: pair.got(three(pair), logprobs=[True, False, True]),
        "penalised_logprobs": lambda: pair.got(three(pair, pen_kw), logprobs=True),
    }

    def plain(r):
        return [x.tolist() if isinstance(x, np.ndarray) and x.dtype != np.float32 else bits(x).tolist() if isinstance(x, np.ndarray) else x for x in r]

    first = {}
    for rnd in range(2):
        for name, fn in calls.items():
            r = plain(fn())
            assert not hip_backend.last_error(), hip_backend.last_error()
            assert first.setdefault(name, r) == r, (rnd, name)
    assert first["sampled"][0] == first["logprobs"][0] and first["penalised"][0] == first["penalised_logprobs"][0]
    print("the penalised calls gave other tokens than the plain ones:", first["sampled"][0] != first["penalised"][0])
    # the first sampled result is the reference's
    pair.check(three(pair), tag="alternation")
    pair.close()


# ── 10. nothing is written behind the tokens ───────────────────────────────────────────────────────────────────────────

def test_nothing_is_written_behind_the_tokens(hip_backend):
    """a raw call with canaries around tokens_out, n_produced and stats; max_tokens = 12 above every count; per_seq = NULL"""
    be, B, Ts, cap = hip_backend, 3, 4, 12
    pair = Pair(be, SD.tiny(), B, Ts, behind=())
    counts = [9, 4, 0]
    sps = [S(**KW[b]) for b in range(B)]
    rq = [BM.Request(FIRST_AT_0, 0, counts[b], sps[b]) for b in range(B)]
    want = pair.want(rq, max_tokens=cap)
    G = 8  # guard words on both sides
    out = np.full(G + B * cap + G, -77, np.int64)
    prod = np.full(G + B + G, 0xDEAD, np.uint32)
    stats = np.full(G + 4 * B + G, 0xBEEF, np.uint32)
    firsts, starts, n = (np.ascontiguousarray(x, np.uint32) for x in ([FIRST_AT_0] * B, [0] * B, counts))
    rc = capi.load_hip().zgml_hip_resident_decode_batch_speculative_sampled(
        be.ctx, pair.s.handle, firsts.ctypes.data_as(u32p), starts.ctypes.data_as(u32p), n.ctypes.data_as(u32p), cap, None, (capi.SamplingC * B)(*sps),
        out[G:].ctypes.data, C.cast(prod[G:].ctypes.data, u32p), C.cast(stats[G:].ctypes.data, C.POINTER(capi.SpecStatsC)))
    assert rc == 0 and not be.last_error(), be.last_error()
    assert np.all(out[:G] == -77) and np.all(out[G + B * cap:] == -77)
    assert np.all(prod[:G] == 0xDEAD) and np.all(prod[G + B:] == 0xDEAD)
    assert np.all(stats[:G] == 0xBEEF) and np.all(stats[G + 4 * B:] == 0xBEEF)
    rows = out[G:G + B * cap].reshape(B, cap)
    assert rows.tolist() == want[0].tolist() and prod[G:G + B].tolist() == want[1] == counts
    for b in range(B):
        assert np.all(rows[b, counts[b]:] == -1)
        assert stats[G + 4 * b:G + 4 * b + 3].tolist() == [want[2][b][k] for k in ("steps", "drafted", "accepted")]
    pair.close()
