"""Speculative decode under batching on the MI355X (zgml_hip_resident_decode_batch_speculative): B sequences on a batched plan with
Ts columns per sequence, every one running the greedy-exact verify loop of zgml_hip_resident_decode_speculative on the device. The
tokens of a sequence are those of plain greedy decode — the decode plan's resident stream — whatever its drafts and whatever the
other sequences of the batch do, and its statistics are exactly what tests/spec_model.py predicts for it alone.

The tie condition of tests/test_hip_spec_decode.py holds here as it does there (asserted on the CPU with the oracle at every run:
oracle_stream): the same first tokens, positions and stream lengths, so no new search. At Llama-2-7B dimensions it cannot hold
(that module's docstring); there the device loop is compared with the same plan driven step by step from the host."""
import ctypes as C
import re

import numpy as np
import pytest

from zgml_amd import capi, llama
from tests import spec_model as SM
from tests import test_hip_spec_decode as SD
from tests.test_hip_l7dims import l7cfg

pytestmark = pytest.mark.gpu

N, T_MAX, PROMPT_LEN = SD.N, SD.T_MAX, SD.PROMPT_LEN
FIRST_AT_0, FIRST_AT_8, FIRST_INT8 = SD.FIRST_AT_0, SD.FIRST_AT_8, SD.FIRST_INT8
u32p = C.POINTER(C.c_uint32)

_decode_streams = {}


def stream_of(be, oracle, kvq, first, start):
    """The decode plan's resident stream of N + T_MAX - 1 tokens (computed once per module), which the tie condition — asserted by
    SD.oracle_stream at every call — promises to be the oracle's"""
    ref = SD.oracle_stream(oracle, kvq, first, start)
    key = (kvq, first, start)
    if key not in _decode_streams:
        _decode_streams[key] = SD.decode_plan_stream(be, SD.tiny(kvq), first, start, N + T_MAX - 1)
    assert _decode_streams[key] == ref[:N + T_MAX - 1]
    return _decode_streams[key]


def batch_session(be, cfg, B, Ts, kvq=0, small_m=True, like=None, threads=8):
    bm = llama.BatchModel(cfg, B, llama.Q4_0, threads=threads, like=like, kv_quant_block=kvq, tokens_per_seq=Ts)
    s = llama.BatchSession(bm, llama.hip_backend_fns(be), B, small_m_matvec=small_m)
    s.resident_setup(be)
    return s, bm


def admit_prompt(be, s, bm, seq, Ts):
    """the PROMPT_LEN-token prompt prefilled on a Ts-token plan of the same weights and handed to sequence `seq` (the last chunk
    overlaps the one before it where Ts does not divide the prompt: the same columns again)"""
    cfg = bm.cfg
    mp = llama.Model(cfg, token_len=Ts, like=bm)
    sp = llama.Session(mp, llama.hip_backend_fns(be))
    p = SD.prompt(cfg)
    for at in sorted({min(c, PROMPT_LEN - Ts) for c in range(0, PROMPT_LEN, Ts)}):
        sp.prefill(p[at:at + Ts], at, want_logits=False)
    s.admit(seq, sp, PROMPT_LEN)
    be.synchronize()
    sp.close(), mp.close()
    return p


def closed_form(form, n, Ts):
    steps = -(-n // Ts)
    if form == "perfect":
        return {"steps": steps, "drafted": steps * (Ts - 1), "accepted": steps * (Ts - 1)}
    if form == "wrong_everywhere":
        return {"steps": n, "drafted": n * (Ts - 1), "accepted": 0}
    return None


@pytest.mark.parametrize("Ts", [2, 4, 5])
def test_tokens_and_stats_of_three_sequences(hip_backend, oracle, Ts):
    """B = 3 (M = 6, 12, 15): sequence 0 and 2 the same request from position 0, sequence 1 behind an admitted prompt; the draft forms
    perfect / n-gram (with the prompt as history where there is one) / wrong everywhere rotate over the sequences"""
    be, cfg, B = hip_backend, SD.tiny(), 3
    firsts, starts, counts = [FIRST_AT_0, FIRST_AT_8, FIRST_AT_0], [0, PROMPT_LEN, 0], [N, 17, N]
    streams = [stream_of(be, oracle, 0, f, st) for f, st in zip(firsts, starts)]
    s, bm = batch_session(be, cfg, B, Ts)
    p = admit_prompt(be, s, bm, 1, Ts)
    hists = [None, p, None]
    forms = ["perfect", "ngram", "wrong_everywhere"]
    for rot in range(3):
        fb = [forms[(b + rot) % 3] for b in range(B)]
        drafts = [SD.drafts_of(fb[b], streams[b], cfg.vocab_size) for b in range(B)]
        toks, stats = s.resident_decode_batch_speculative(firsts, starts, counts, histories=hists, drafts=drafts)
        assert not be.last_error(), be.last_error()
        print(Ts, fb, stats)
        assert toks.shape == (B, N)
        for b in range(B):
            assert toks[b, :counts[b]].tolist() == streams[b][:counts[b]], (fb, b)
            assert np.all(toks[b, counts[b]:] == -1)
            want = SM.predict(streams[b], firsts[b], starts[b], counts[b], Ts, history=hists[b], drafts=drafts[b])
            assert stats[b] == want, (fb, b, stats[b], want)
            if closed_form(fb[b], counts[b], Ts):
                assert stats[b] == closed_form(fb[b], counts[b], Ts), (fb, b)
        # sequences 0 and 2: one request, other drafts — the same tokens; perfect against wrong drafts: other step counts
        assert toks[0].tolist() == toks[2].tolist()
        if {fb[0], fb[2]} == {"perfect", "wrong_everywhere"}:
            assert stats[0]["steps"] != stats[2]["steps"]
    s.close(), bm.close()


def test_two_calls_equal_one_raggedly(hip_backend, oracle):
    """(10, 5, 24) tokens, then sequences 0 and 1 continue while sequence 2 wants nothing: the streams are those of one call, and the
    idle sequence keeps its row, its statistics and its cache (a third call continues it)"""
    be, cfg, B, Ts = hip_backend, SD.tiny(), 3, 4
    firsts, starts = [FIRST_AT_0, FIRST_AT_8, FIRST_AT_0], [0, PROMPT_LEN, 0]
    streams = [stream_of(be, oracle, 0, f, st) for f, st in zip(firsts, starts)]
    s, bm = batch_session(be, cfg, B, Ts)
    p = admit_prompt(be, s, bm, 1, Ts)
    perfect = SD.drafts_of("perfect", streams[1], cfg.vocab_size)
    a, st_a = s.resident_decode_batch_speculative(firsts, starts, [10, 5, N], histories=[None, p, None], drafts=[None, perfect, None])
    assert not be.last_error(), be.last_error()
    for b, n in enumerate([10, 5, N]):
        assert a[b, :n].tolist() == streams[b][:n] and np.all(a[b, n:] == -1)
    first2 = [int(a[0, 9]), int(a[1, 4]), int(a[2, N - 1])]
    start2 = [10, PROMPT_LEN + 5, N]
    hist2 = [[FIRST_AT_0] + a[0, :9].tolist(), p + [FIRST_AT_8] + a[1, :4].tolist(), None]
    b2, st_b = s.resident_decode_batch_speculative(first2, start2, [14, 12, 0], histories=hist2, drafts=[None, perfect[5:], None])
    assert not be.last_error(), be.last_error()
    assert a[0, :10].tolist() + b2[0, :14].tolist() == streams[0][:24]
    assert a[1, :5].tolist() + b2[1, :12].tolist() == streams[1][:17]
    assert np.all(b2[2] == -1) and np.all(b2[1, 12:] == -1)
    assert st_b[2] == {"steps": 0, "drafted": 0, "accepted": 0}
    assert st_b[0] == SM.predict(streams[0][10:], first2[0], 10, 14, Ts, history=hist2[0])
    assert st_b[1] == SM.predict(streams[1][5:], first2[1], PROMPT_LEN + 5, 12, Ts, history=hist2[1], drafts=perfect[5:])
    # the idle sequence's cache in front of its end position is intact: it continues, the others idle behind their own ends
    c, _ = s.resident_decode_batch_speculative([int(b2[0, 13]), int(b2[1, 11]), first2[2]], [24, PROMPT_LEN + 17, N], [0, 0, 3])
    assert not be.last_error(), be.last_error()
    assert c[2].tolist() == streams[2][N:N + 3] and np.all(c[:2] == -1)
    s.close(), bm.close()


def raw_call(be, s, first, start, n, max_tokens, opts, out, stats):
    a = [None if x is None else np.ascontiguousarray(x, dtype=np.uint32) for x in (first, start, n)]
    ptr = [None if x is None else x.ctypes.data_as(u32p) for x in a]
    return capi.load_hip().zgml_hip_resident_decode_batch_speculative(be.ctx, s.handle, ptr[0], ptr[1], ptr[2], max_tokens, opts,
                                                                      None if out is None else out.ctypes.data, stats)


def test_nothing_is_written_behind_the_tokens(hip_backend, oracle):
    """max_tokens = 12 above every count: row b is its tokens, then -1 up to max_tokens, and the canaries behind the B rows stay;
    per_seq = NULL (lookup, ngram 2, no history) and stats = NULL are accepted"""
    be, cfg, B, Ts, cap = hip_backend, SD.tiny(), 3, 4, 12
    stream = stream_of(be, oracle, 0, FIRST_AT_0, 0)
    s, bm = batch_session(be, cfg, B, Ts)
    counts = [9, 4, 0]
    out = np.full(B * cap + 8, -77, np.int64)
    assert raw_call(be, s, [FIRST_AT_0] * B, [0] * B, counts, cap, None, out, None) == 0 and not be.last_error(), be.last_error()
    rows = out[:B * cap].reshape(B, cap)
    for b in range(B):
        assert rows[b, :counts[b]].tolist() == stream[:counts[b]] and np.all(rows[b, counts[b]:] == -1)
    assert np.all(out[B * cap:] == -77)
    # the same through the wrapper, with statistics: those of the lookup without history
    toks, stats = s.resident_decode_batch_speculative([FIRST_AT_0] * B, [0] * B, counts)
    assert toks.tolist() == rows[:, :9].tolist()
    assert stats[:2] == [SM.predict(stream, FIRST_AT_0, 0, n, Ts) for n in counts[:2]] and stats[2] == {"steps": 0, "drafted": 0, "accepted": 0}
    s.close(), bm.close()


def test_int8_kv_equals_the_oracle(hip_backend, oracle):
    be, cfg, B, Ts = hip_backend, SD.tiny(), 2, 4
    stream = stream_of(be, oracle, 32, FIRST_INT8, 0)  # (the decode plan and the oracle with cfg.kv_quant_block = 32)
    s, bm = batch_session(be, cfg, B, Ts, kvq=32)
    for fb in (["perfect", "wrong_everywhere"], ["ngram", "wrong_at_two"]):
        drafts = [SD.drafts_of(f, stream, cfg.vocab_size) for f in fb]
        toks, stats = s.resident_decode_batch_speculative([FIRST_INT8] * B, [0] * B, [N, 17], drafts=drafts)
        assert not be.last_error(), be.last_error()
        print(fb, stats)
        for b, n in enumerate([N, 17]):
            assert toks[b, :n].tolist() == stream[:n] and np.all(toks[b, n:] == -1)
            assert stats[b] == SM.predict(stream, FIRST_INT8, 0, n, Ts, drafts=drafts[b]), (fb, b)
            if closed_form(fb[b], n, Ts):
                assert stats[b] == closed_form(fb[b], n, Ts)
    s.close(), bm.close()


def test_refusals_enqueue_nothing_and_leave_the_program_usable(hip_backend):
    be, cfg, B, Ts = hip_backend, SD.tiny(), 2, 4
    hip, V, S = capi.load_hip(), cfg.vocab_size, cfg.max_seq_len
    s, bm = batch_session(be, cfg, B, Ts)
    before = SD._dispatches(be, s.handle)

    def refused(call, text):
        with pytest.raises(RuntimeError, match=text):
            call()
        hip.zgml_hip_clear_error(be.ctx)
        assert SD._dispatches(be, s.handle) == before, text

    def raw_refused(text, *args):
        assert raw_call(be, s, *args) == -1
        assert re.search(text, be.last_error()), (text, be.last_error())
        hip.zgml_hip_clear_error(be.ctx)
        assert SD._dispatches(be, s.handle) == before, text

    bad = [  # (first, start, n, histories, drafts, ngram), the text: every sequence is held to the single-sequence call's rules
        (([1, V], [0, 0], [4, 4], None, None, 2), r"sequence 1.*token out of range"),
        (([V, 1], [0, 0], [0, 4], None, None, 2), r"sequence 0.*token out of range"),   # (also one that wants nothing: it runs its token)
        (([1, 1], [0, 2], [4, 4], [None, [1, V]], None, 2), r"sequence 1.*token out of range"),
        (([1, 1], [0, 0], [4, 4], None, [[1, 2, V], None], 2), r"sequence 0.*token out of range"),
        (([1, 1], [0, 3], [4, 4], [None, [1, 2]], None, 2), r"sequence 1.*n_history"),
        (([1, 1], [0, 0], [4, 4], None, None, 5), "ngram"),
        (([1, 1], [0, S - Ts - 3], [4, 4], None, None, 2), r"sequence 1.*max_seq"),     # start + n + Ts = max_seq + 1
        (([1, 1], [0, S - Ts + 1], [4, 0], None, None, 2), r"sequence 1.*max_seq"),     # ... of a sequence that only idles
        (([1, 1], [0, 0], [S - Ts + 1, 1], None, None, 2), r"sequence 0.*max_seq"),
    ]
    for args, text in bad:
        refused(lambda: s.resident_decode_batch_speculative(*args[:3], histories=args[3], drafts=args[4], ngram=args[5]), text)
    out = np.full(B * 4, -77, np.int64)
    opts = (capi.SpecDecodeC * B)()
    opts[1].mode = 2
    raw_refused(r"sequence 1.*mode", [1, 1], [0, 0], [4, 4], 4, opts, out, None)
    raw_refused(r"sequence 0.*max_tokens", [1, 1], [0, 0], [5, 2], 4, None, out, None)
    raw_refused("NULL", None, [0, 0], [4, 4], 4, None, out, None)
    raw_refused("NULL", [1, 1], None, [4, 4], 4, None, out, None)
    raw_refused("NULL", [1, 1], [0, 0], None, 4, None, out, None)
    raw_refused("NULL", [1, 1], [0, 0], [4, 4], 4, None, None, None)
    assert np.all(out == -77)  # a refused call writes no token either
    # a constraint attached to any sequence
    con = be.constraint_create(np.zeros(V, np.uint16), np.zeros((1, 1), np.uint16))
    s.set_constraint(con, 0, seq=1)
    refused(lambda: s.resident_decode_batch_speculative([1, 1], [0, 0], [4, 4]), "constraint is attached")
    s.set_constraint(None, seq=1)
    be.constraint_free(con)
    # all counts zero: 0, nothing touched
    toks, stats = s.resident_decode_batch_speculative([1, 1], [0, 0], [0, 0])
    assert toks.shape == (B, 0) and all(st == {"steps": 0, "drafted": 0, "accepted": 0} for st in stats) and SD._dispatches(be, s.handle) == before
    # the one-token-per-sequence loops refuse this plan, naming the call that runs it
    refused(lambda: s.resident_decode_batch([1, 1], [0, 0], [2, 2]), "resident_decode_batch_speculative")
    prod = np.zeros(B, np.uint32)
    two = np.ones(B, np.uint32)
    assert hip.zgml_hip_resident_decode_batch_sampled(be.ctx, s.handle, two.ctypes.data_as(u32p), two.ctypes.data_as(u32p), two.ctypes.data_as(u32p), 2, None,
                                                      out.ctypes.data, prod.ctypes.data_as(u32p)) == -1
    assert "resident_decode_batch_speculative" in be.last_error() and SD._dispatches(be, s.handle) == before
    hip.zgml_hip_clear_error(be.ctx)
    # this call refuses a plan with one column per sequence, and a plain plan
    s1, bm1 = batch_session(be, cfg, B, 1, like=bm)
    assert raw_call(be, s1, [1, 1], [0, 0], [4, 4], 4, None, out, None) == -1 and "one column per sequence" in be.last_error()
    hip.zgml_hip_clear_error(be.ctx)
    sp, mp = SD.spec_session(be, cfg, Ts)
    assert raw_call(be, sp, [1, 1], [0, 0], [4, 4], 4, None, out, None) == -1 and "not a batched program" in be.last_error()
    hip.zgml_hip_clear_error(be.ctx)
    # ... and the single-sequence call still refuses every batched plan
    one = np.zeros(4, np.int64)
    assert hip.zgml_hip_resident_decode_speculative(be.ctx, s.handle, 1, 0, 4, None, one.ctypes.data, None) == -1 and "batched" in be.last_error()
    hip.zgml_hip_clear_error(be.ctx)
    # the edge that is allowed: start + n + Ts == max_seq
    toks, _ = s.resident_decode_batch_speculative([1, 1], [S - Ts - 4, 0], [4, S - Ts])
    assert toks.shape == (B, S - Ts) and np.all(toks[0, :4] >= 0) and np.all(toks[1] >= 0) and not be.last_error(), be.last_error()
    # ... and the program still steps through the vtable, like a fresh session's
    fresh = llama.BatchSession(bm, llama.hip_backend_fns(be), B)
    toks8, pos = [(5 * i + 2) % V for i in range(B * Ts)], [0, 0]  # (from position 0: no column of an earlier call is read)
    n_a, l_a = s.step(toks8, pos)
    n_b, l_b = fresh.step(toks8, pos)
    assert n_a.tolist() == n_b.tolist() and np.array_equal(l_a, l_b) and not be.last_error(), be.last_error()
    for x in (fresh, s1, bm1, sp, mp, s, bm):
        x.close()


@pytest.fixture(scope="module")
def l7_base():
    m = llama.Model(l7cfg(2), llama.Q4_0, threads=16)
    yield m
    m.close()


@pytest.mark.parametrize("small_m", [1, 0])
def test_l7_dimensions_device_loop_equals_the_host_driven_loop(hip_backend, l7_base, small_m):
    """Two layers at Llama-2-7B dimensions, B = 2, Ts = 4 (M = 8), 12 tokens per sequence, compiled with ZGML_HIP_OPT_SMALL_M_MATVEC 1 and 0
    (at M = 8 the value 1 is past the row kernel's measured bound of six rows, so both take the tile kernels today: the two runs
    pin that the option changes nothing it should not). The reference is the same plan driven from the host: per sequence the
    model's loop (SM.spec_loop) with every verify step one BatchSession.step over the B * Ts tokens — the other sequence's columns
    run token 0 at position 0 in their own slab — and all rows read back. Same kernels, same inputs: tokens and statistics identical,
    for n-gram drafts and for provided drafts right and wrong at two places."""
    be, B, Ts, n = hip_backend, 2, 4, 12
    firsts = [20000, 4321]
    cfg = l7_base.cfg
    s, bm = batch_session(be, cfg, B, Ts, small_m=small_m, like=l7_base)
    print("small_m", small_m, "row-kernel launches:", be.planText(s.handle).count("qmatvec-kon-rows"))  # (value 1 takes it up to M = 6 only)
    host = llama.BatchSession(bm, llama.hip_backend_fns(be), B, small_m_matvec=small_m)

    def rows_of(b):
        def rows(c, pos):
            toks, at = [0] * (B * Ts), [0] * B
            toks[b * Ts:(b + 1) * Ts], at[b] = c, pos
            nxt, _ = host.step(toks, at)
            return nxt[b * Ts:(b + 1) * Ts]
        return rows

    want = [SM.spec_loop(rows_of(b), firsts[b], 0, n, Ts)[0] for b in range(B)]
    right = [w + w[-1:] * Ts for w in want]
    wrong = [[(t + 1) % cfg.vocab_size if i in (2, 7) else t for i, t in enumerate(r)] for r in right]
    for drafts in ([None, None], right, [wrong[0], None], [right[0], wrong[1]]):
        want_stats = []
        for b in range(B):
            w, st = SM.spec_loop(rows_of(b), firsts[b], 0, n, Ts, drafts=drafts[b])
            assert w == want[b]
            want_stats.append(st)
        toks, stats = s.resident_decode_batch_speculative(firsts, [0] * B, [n] * B, drafts=drafts)
        assert not be.last_error(), be.last_error()
        print(small_m, stats)
        assert toks.tolist() == want and stats == want_stats
    host.close(), s.close(), bm.close()


@pytest.mark.parametrize("B", [2, 4])
def test_plan_shape_one_attention_launch_per_layer(hip_backend, l7_base, B):
    """f32 KV at Llama-2-7B dimensions, Ts = 4: the planner groups the B * 32 attention ops of a layer (seq_q = 4 each) into one
    launch, as it groups the 32 of a token_len = 4 plan"""
    from tests.test_hip_batch_decode import launches
    L, Ts = 2, 4
    bm = llama.BatchModel(None, B, like=l7_base, tokens_per_seq=Ts)
    s = llama.BatchSession(bm, llama.hip_backend_fns(hip_backend), B)
    text = hip_backend.planText(s.handle)
    ls = launches(text)
    att = [l for l in ls if l[0] == capi.DOP["attention"]]
    print(f"B = {B}, Ts = {Ts}: {len(ls)} launches, {(len(ls) - 2) / L:g} per layer, attention launches {[(l[1], l[4].strip()) for l in att]}")
    assert len(att) == L, text
    H = bm.cfg.n_heads
    assert all(l[1] >= B * H for l in att), text  # every head of every sequence (with whatever stores are folded into it)
    s.close(), bm.close()
