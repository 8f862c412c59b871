"""Sampled speculative decode on the MI355X (zgml_hip_resident_decode_speculative_sampled): the verify step of a token_len = T
plan with seeded top-k / top-p picks instead of first maxima, entirely on the device.

THE REFERENCE everywhere is the SAME T-plan driven from the host: Session.prefill(c, pos) through the vtable, all T logits rows
downloaded, every row sampled by zgml_amd/csrc/sample.h (tests/cpp/sample_probe.cpp: c_sample(row_j, sp, pos + j)), and the loop of
the Python model tests/spec_sampled_model.py. Same kernels, same inputs: bit-exact token equality and equal statistics, no
tolerance and no tie condition. The decode plan (token_len = 1) is not a reference here: its M = 1 kernels agree with the T-plan's
to the parity bar only (include/zgml_hip.h says what that means for the two streams).

Every reference is computed once per module, from the reference alone, and left unchanged; the preconditions — it does sample,
"wrong" drafts are wrong where meant, the stream is long enough for the last step's drafts — are asserted on it before the
device loop is asked."""
import ctypes as C

import numpy as np
import pytest

from zgml_amd import capi, llama
from tests import spec_model as SM
from tests import spec_sampled_model as SSM
from tests.test_hip_l7dims import l7cfg
from tests.test_hip_sample import PARAMS
from tests.test_hip_spec_decode import FIRST_AT_0, FIRST_AT_8, FORMS, N, PROMPT_LEN, _dispatches, _download, drafts_of, prompt, spec_session, tiny
from tests.test_sample_host import c_sample

pytestmark = pytest.mark.gpu
S = capi.SamplingC.of


class Host:
    """The reference side: a T-plan of its own stepped through the vtable (behind `start` prompt tokens), and the streams it gave."""

    def __init__(self, be, cfg, T, start, small_m=None, threads=8):
        self.be, self.cfg, self.T = be, cfg, T
        self.s, self.m = spec_session(be, cfg, T, small_m=small_m, threads=threads)
        p = prompt(cfg, start)
        for at in range(0, start, T):
            self.s.prefill(p[at:at + T], at, want_logits=False)
        self.streams = {}

    def rows_fn(self, sp):
        T, V = self.T, self.cfg.vocab_size

        def rows(c, pos):
            self.s.prefill(c, pos, want_logits=False)
            logits = _download(self.be, self.s.handle, self.m.buf("logits"), T * V).reshape(T, V)
            return [c_sample(logits[j], sp, pos + j) for j in range(T)]
        return rows

    def stream(self, sp, first, start, n):
        """n tokens of the generation under sp, from a run of the model's loop without any draft"""
        key = (sp.temperature, sp.top_p, sp.top_k, sp.seed, sp.stream, first, start, n)
        if key not in self.streams:
            toks, produced, _ = SSM.spec_loop(self.rows_fn(sp), first, start, n, self.T, drafts=[])
            assert produced == n
            self.streams[key] = toks
        return list(self.streams[key])

    def close(self):
        self.s.close(), self.m.close()


@pytest.fixture(scope="module")
def hosts(hip_backend):
    made = {}

    def get(T, start=0):
        if (T, start) not in made:
            made[(T, start)] = Host(hip_backend, tiny(), T, start)
        return made[(T, start)]
    yield get
    for h in made.values():
        h.close()


def check_forms(be, s, cfg, T, sp, first, start, stream, history, forms=FORMS):
    assert len(stream) == N + T - 1  # precondition: perfect drafts exist for the last step
    for form in forms:
        drafts = drafts_of(form, stream, cfg.vocab_size)
        if form == "wrong_everywhere":
            assert all(d != t for d, t in zip(drafts, stream))
        if form == "wrong_at_two":
            assert [i for i, (d, t) in enumerate(zip(drafts, stream)) if d != t] == [5, 14]
        toks, produced, stats = s.resident_decode_speculative_sampled(first, start, N, sp, history=history, drafts=drafts)
        assert not be.last_error(), be.last_error()
        want = SM.predict(stream, first, start, N, T, history=history, drafts=drafts)
        print(T, start, form, stats)
        assert toks.tolist() == stream[:N] and produced == N, form
        assert stats == want, (form, stats, want)
        steps = -(-N // T)
        if form == "perfect":
            assert stats == {"steps": steps, "drafted": steps * (T - 1), "accepted": steps * (T - 1)}
        if form == "wrong_everywhere":
            assert stats == {"steps": N, "drafted": N * (T - 1), "accepted": 0}


# ── 1. all forms, tiny model ───────────────────────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("name", ["k40_p95", "k256_p1"])
@pytest.mark.parametrize("T", [2, 4, 5])
def test_tokens_and_stats_from_position_0(hip_backend, hosts, T, name):
    cfg, sp = tiny(), S(seed=1234, stream=0, **PARAMS[name])
    stream = hosts(T).stream(sp, FIRST_AT_0, 0, N + T - 1)
    assert len(set(stream)) > 3  # precondition: it does sample
    s, m = spec_session(hip_backend, cfg, T)
    check_forms(hip_backend, s, cfg, T, sp, FIRST_AT_0, 0, stream, None)
    s.close(), m.close()


@pytest.mark.parametrize("name", ["k40_p95", "k256_p1"])
def test_tokens_and_stats_behind_a_prefilled_prompt(hip_backend, hosts, name):
    """T = 4 from position 8: two resident_prefill chunks of the same plan fill the cache, the prompt is handed over as history"""
    cfg, T, sp = tiny(), 4, S(seed=1234, stream=0, **PARAMS[name])
    stream = hosts(T, PROMPT_LEN).stream(sp, FIRST_AT_8, PROMPT_LEN, N + T - 1)
    assert len(set(stream)) > 3
    s, m = spec_session(hip_backend, cfg, T)
    p = prompt(cfg)
    for chunk in range(PROMPT_LEN // T):
        s.resident_prefill(p[chunk * T:(chunk + 1) * T], chunk * T)
    check_forms(hip_backend, s, cfg, T, sp, FIRST_AT_8, PROMPT_LEN, stream, p)
    # without the history the lookup sees only this call's tokens: the same tokens, its own statistics
    toks, produced, stats = s.resident_decode_speculative_sampled(FIRST_AT_8, PROMPT_LEN, N, sp)
    assert toks.tolist() == stream[:N] and produced == N and stats == SM.predict(stream, FIRST_AT_8, PROMPT_LEN, N, T)
    s.close(), m.close()


def test_the_whole_flow_prefill_then_sample_then_speculate(hip_backend, hosts):
    """resident_prefill leaves the chunk's logits rows in the buffer: the first token is zgml_hip_sample over the LAST row at the
    position of that row, start - 1; the sampled loop goes on from it at `start`"""
    cfg, T, sp = tiny(), 4, S(seed=5, stream=2, **PARAMS["k40_p95"])
    V, p = cfg.vocab_size, prompt(cfg)
    host = hosts(T, PROMPT_LEN)
    host.s.prefill(p[PROMPT_LEN - T:], PROMPT_LEN - T, want_logits=False)
    last = _download(hip_backend, host.s.handle, host.m.buf("logits"), T * V).reshape(T, V)[T - 1]
    first = c_sample(last, sp, PROMPT_LEN - 1)
    stream = host.stream(sp, first, PROMPT_LEN, N + T - 1)
    s, m = spec_session(hip_backend, cfg, T)
    for chunk in range(PROMPT_LEN // T):
        s.resident_prefill(p[chunk * T:(chunk + 1) * T], chunk * T)
    tok, _ = hip_backend.sample(s.handle, m.buf("logits"), (T - 1) * V, V, sp, PROMPT_LEN - 1)
    assert tok == first
    toks, produced, _ = s.resident_decode_speculative_sampled(tok, PROMPT_LEN, N, sp, history=p)
    assert toks.tolist() == stream[:N] and produced == N and not hip_backend.last_error()
    s.close(), m.close()


# ── 2. top_k = 1 is the greedy form ────────────────────────────────────────────────────────────────────────────────────

def test_top_k_1_equals_the_greedy_speculative_loop_on_the_same_program(hip_backend):
    cfg, T, sp = tiny(), 4, S(seed=99, stream=3, **PARAMS["k1"])
    s, m = spec_session(hip_backend, cfg, T)
    stream = s.resident_decode_speculative(FIRST_AT_0, 0, N + T - 1)[0].tolist()
    for form in FORMS:
        drafts = drafts_of(form, stream, cfg.vocab_size)
        g_toks, g_stats = s.resident_decode_speculative(FIRST_AT_0, 0, N, drafts=drafts)
        toks, produced, stats = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, N, sp, drafts=drafts)
        assert not hip_backend.last_error(), hip_backend.last_error()
        assert g_toks.tolist() == stream[:N]
        assert toks.tolist() == g_toks.tolist() and produced == N and stats == g_stats, form
    s.close(), m.close()


# ── 3. seeds and streams ───────────────────────────────────────────────────────────────────────────────────────────────

def test_seed_and_stream(hip_backend, hosts):
    cfg, T = tiny(), 4
    sps = [S(seed=1, stream=0, **PARAMS["k256_p1"]), S(seed=2, stream=0, **PARAMS["k256_p1"]), S(seed=1, stream=1, **PARAMS["k256_p1"]),
           S(seed=1 << 32, stream=0, **PARAMS["k256_p1"])]  # (the last: the seed's high word is a key word of its own)
    wants = [hosts(T).stream(sp, FIRST_AT_0, 0, N + T - 1) for sp in sps]
    for i in range(len(wants)):
        for j in range(i):
            assert wants[i][:N] != wants[j][:N], (i, j)  # precondition: seeds and streams matter to the reference
    s, m = spec_session(hip_backend, cfg, T)
    for sp, want in zip(sps, wants):  # (one captured graph, four parameter sets)
        check_forms(hip_backend, s, cfg, T, sp, FIRST_AT_0, 0, want, None, forms=("perfect", "ngram"))
    s.close(), m.close()


# ── 4. two calls equal one ─────────────────────────────────────────────────────────────────────────────────────────────

def test_two_calls_equal_one(hip_backend, hosts):
    """10 + 14 tokens, the second call continuing from the first call's last token and position with the concatenated history"""
    cfg, T, sp = tiny(), 4, S(seed=1234, stream=0, **PARAMS["k40_p95"])
    stream = hosts(T).stream(sp, FIRST_AT_0, 0, N + T - 1)
    s, m = spec_session(hip_backend, cfg, T)
    for form in ("ngram", "perfect", "wrong_at_two"):
        drafts = drafts_of(form, stream, cfg.vocab_size)
        one, _, _ = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, N, sp, drafts=drafts)
        a, na, _ = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, 10, sp, drafts=drafts)
        hist = [FIRST_AT_0] + a[:9].tolist()
        b, nb, _ = s.resident_decode_speculative_sampled(int(a[9]), 10, 14, sp, history=hist, drafts=None if drafts is None else drafts[10:])
        assert not hip_backend.last_error(), hip_backend.last_error()
        assert (na, nb) == (10, 14) and a.tolist() + b.tolist() == one.tolist() == stream[:N], form
    s.close(), m.close()


# ── 5. a stop token in the middle of a step ────────────────────────────────────────────────────────────────────────────

def test_stop_token_mid_step(hip_backend, hosts):
    cfg, T, V = tiny(), 4, tiny().vocab_size
    # a reference stream whose token at index 5 — the second token of step 2 under perfect drafts — is new to the stream
    for seed in range(16):
        sp = S(seed=seed, **PARAMS["k256_p1"])
        want = hosts(T).stream(sp, FIRST_AT_0, 0, N + T - 1)
        if want[5] not in want[:5]:
            break
    else:
        pytest.fail("no reference stream emits a new token at index 5")
    stop = want[5]
    sp_stop = S(seed=seed, stop=[stop], **PARAMS["k256_p1"])
    s, m = spec_session(hip_backend, cfg, T)
    got, produced, stats = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, N, sp_stop, drafts=want)
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert produced == 6 and got[:6].tolist() == want[:6] and np.all(got[6:] == -1)
    assert stats["steps"] == 2 and stats["accepted"] == 2 * (T - 1)  # (accepted counts before the cut)
    assert (got.tolist(), produced, stats) == SSM.spec_loop(SM.stream_rows(want, FIRST_AT_0, 0), FIRST_AT_0, 0, N, T, drafts=want, stop=[stop])
    # from the stop position the generation continues as the reference does
    nxt, n2, _ = s.resident_decode_speculative_sampled(stop, 6, 10, sp, history=[FIRST_AT_0] + want[:5], drafts=want[6:])
    assert n2 == 10 and nxt.tolist() == want[6:16]
    # the same stop under drafts that are wrong everywhere: the same 6 tokens, one per step
    got, produced, stats = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, N, sp_stop, drafts=drafts_of("wrong_everywhere", want, V))
    assert produced == 6 and got[:6].tolist() == want[:6] and np.all(got[6:] == -1) and stats["steps"] == 6
    # ... and under n-gram drafts
    got, produced, _ = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, N, sp_stop)
    assert produced == 6 and got[:6].tolist() == want[:6] and np.all(got[6:] == -1)
    # a stop token that is the last wanted token: nothing is left to cut
    got, produced, _ = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, 6, sp_stop, drafts=want)
    assert produced == 6 and got.tolist() == want[:6]
    assert not hip_backend.last_error(), hip_backend.last_error()
    s.close(), m.close()


# ── 6. alternation on one program ──────────────────────────────────────────────────────────────────────────────────────

def test_greedy_sampled_and_prefill_alternate_on_one_program(hip_backend, hosts):
    cfg, T, sp = tiny(), 4, S(seed=77, **PARAMS["k40_p95"])
    want = hosts(T).stream(sp, FIRST_AT_0, 0, N + T - 1)
    s, m = spec_session(hip_backend, cfg, T)
    chunk = prompt(cfg, T)
    g1 = s.resident_decode_speculative(FIRST_AT_0, 0, N)
    a1 = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, N, sp)
    p1 = s.resident_prefill(chunk, 0)
    a2 = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, N, sp)
    g2 = s.resident_decode_speculative(FIRST_AT_0, 0, N)
    p2 = s.resident_prefill(chunk, 0)
    a3 = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, N, sp, drafts=want)
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert g1[0].tolist() == g2[0].tolist() and g1[1] == g2[1] and p1 == p2
    assert a1[0].tolist() == a2[0].tolist() == a3[0].tolist() == want[:N] and a1[1:] == a2[1:]
    # a longer call regrows the token table, which frees both graphs: both loops capture again and give what they gave
    n2 = N + 8
    want2 = hosts(T).stream(sp, FIRST_AT_0, 0, n2)
    b, nb, _ = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, n2, sp)
    g3 = s.resident_decode_speculative(FIRST_AT_0, 0, N)
    assert b.tolist() == want2 and nb == n2 and want2[:N] == want[:N] and g3[0].tolist() == g1[0].tolist() and not hip_backend.last_error()
    s.close(), m.close()


# ── 7. refusals ────────────────────────────────────────────────────────────────────────────────────────────────────────

BAD_PARAMS = [(dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"), (dict(temperature=float("nan")), "temperature"),
              (dict(top_p=0.0), "top_p"), (dict(top_p=1.5), "top_p"), (dict(top_p=float("nan")), "top_p"), (dict(top_k=257), "top_k"),
              (dict(stop=[1, 2, 3, 4, 5]), "n_stop")]


def test_refusals_enqueue_nothing_and_the_next_call_works(hip_backend, hosts):
    cfg, T = tiny(), 4
    hip, V, L = capi.load_hip(), cfg.vocab_size, cfg.max_seq_len
    s, m = spec_session(hip_backend, cfg, T)
    good = S(seed=1, **PARAMS["k40_p95"])
    before = _dispatches(hip_backend, s.handle)

    def refused(call, text):
        with pytest.raises(RuntimeError, match=text):
            call()
        hip.zgml_hip_clear_error(hip_backend.ctx)
        assert _dispatches(hip_backend, s.handle) == before, text

    # what zgml_hip_resident_decode_speculative refuses, with its texts
    for args, text in [((V, 0, 4, None, None, 2), "token out of range"), ((1, 2, 4, [1, V], None, 2), "token out of range"),
                       ((1, 0, 4, None, [1, 2, V], 2), "token out of range"), ((1, 3, 4, [1, 2], None, 2), "n_history"),
                       ((1, 0, 4, None, None, 5), "ngram"), ((1, 0, L - T + 2, None, None, 2), "max_seq"), ((1, L - T - 2, 4, None, None, 2), "max_seq")]:
        refused(lambda: s.resident_decode_speculative_sampled(*args[:3], good, history=args[3], drafts=args[4], ngram=args[5]), text)
    # what the sampling parameters are refused for, with sampling_params' texts
    for kw, text in BAD_PARAMS + [(dict(stop=[V]), "stop token")]:
        refused(lambda: s.resident_decode_speculative_sampled(1, 0, 4, S(**kw)), text)
    # mode > 1 and sampling = NULL: only the C entry point can be asked
    out, n_out, stats = np.zeros(4, np.int64), C.c_uint32(7), capi.SpecStatsC()
    opt = capi.SpecDecodeC(None, 0, 2, None, 0, 0)
    assert hip.zgml_hip_resident_decode_speculative_sampled(hip_backend.ctx, s.handle, 1, 0, 4, C.byref(opt), C.byref(good), out.ctypes.data, C.byref(n_out), C.byref(stats)) == -1
    assert "mode" in hip_backend.last_error() and n_out.value == 0
    hip.zgml_hip_clear_error(hip_backend.ctx)
    assert hip.zgml_hip_resident_decode_speculative_sampled(hip_backend.ctx, s.handle, 1, 0, 4, None, None, out.ctypes.data, None, None) == -1
    assert "no sampling parameters" in hip_backend.last_error()
    hip.zgml_hip_clear_error(hip_backend.ctx)
    assert _dispatches(hip_backend, s.handle) == before
    # no tokens wanted: 0, nothing touched
    toks, produced, stats = s.resident_decode_speculative_sampled(1, 0, 0, good)
    assert toks.size == 0 and produced == 0 and stats == {"steps": 0, "drafted": 0, "accepted": 0} and _dispatches(hip_backend, s.handle) == before
    # a token_len = 1 plan and a batched plan
    m1 = llama.Model(cfg, llama.Q4_0)
    s1 = llama.Session(m1, llama.hip_backend_fns(hip_backend))
    s1.resident_setup(hip_backend)
    before1 = _dispatches(hip_backend, s1.handle)
    with pytest.raises(RuntimeError, match="token_len = 1"):
        s1.resident_decode_speculative_sampled(1, 0, 4, good)
    hip.zgml_hip_clear_error(hip_backend.ctx)
    assert _dispatches(hip_backend, s1.handle) == before1
    assert s1.resident_decode_sampled(1, 0, 4, good)[1] == 4 and not hip_backend.last_error()  # (its own sampled loop still works)
    bm = llama.BatchModel(cfg, 2)
    sb = llama.BatchSession(bm, llama.hip_backend_fns(hip_backend), 2)
    sb.resident_setup(hip_backend)
    before_b = _dispatches(hip_backend, sb.handle)
    assert hip.zgml_hip_resident_decode_speculative_sampled(hip_backend.ctx, sb.handle, 1, 0, 4, None, C.byref(good), out.ctypes.data, None, None) == -1
    assert "batched" in hip_backend.last_error()
    hip.zgml_hip_clear_error(hip_backend.ctx)
    assert _dispatches(hip_backend, sb.handle) == before_b
    assert np.all(sb.resident_decode_batch([1, 2], [0, 0], 4) >= 0) and not hip_backend.last_error()  # (its own loop still works)
    # the edge that is allowed: start + n + T - 1 == max_seq (the last step may store the cache's last column)
    toks, produced, _ = s.resident_decode_speculative_sampled(1, L - T - 3, 4, good, drafts=[])
    assert toks.size == 4 and produced == 4 and np.all(toks >= 0) and not hip_backend.last_error(), hip_backend.last_error()
    # ... and a valid call gives what the reference gives; opt = NULL and the optional outputs NULL are allowed
    want = hosts(T).stream(good, FIRST_AT_0, 0, N + T - 1)
    toks, produced, _ = s.resident_decode_speculative_sampled(FIRST_AT_0, 0, N, good)
    assert toks.tolist() == want[:N] and produced == N
    out = np.full(N, -7, np.int64)
    assert hip.zgml_hip_resident_decode_speculative_sampled(hip_backend.ctx, s.handle, FIRST_AT_0, 0, N, None, C.byref(good), out.ctypes.data, None, None) == 0
    assert out.tolist() == want[:N] and not hip_backend.last_error()
    for x in (s, m, s1, m1, sb, bm):
        x.close()


# ── 9. the neighbours keep their results ───────────────────────────────────────────────────────────────────────────────

def test_the_other_sampled_entry_points_keep_their_results_beside_it(hip_backend):
    """zgml_hip_sample, resident_decode_sampled and resident_decode_batch_sampled share the select / merge kernels with the verify
    step: each gives its reference (the header's pick over the same logits; test_hip_sample.py's host loop) before a sampled
    speculative call in the same context and the same tokens after it"""
    from tests import test_hip_sample as THS
    cfg, T, sp = tiny(), 4, S(seed=1234, stream=0, **PARAMS["k40_p95"])
    V = cfg.vocab_size
    want = THS.host_loop(hip_backend, sp)
    assert len(set(want)) > 3  # precondition: it does sample
    s1, m1 = THS.resident(hip_backend)
    bm = llama.BatchModel(cfg, 2)
    sb = llama.BatchSession(bm, llama.hip_backend_fns(hip_backend), 2)
    sb.resident_setup(hip_backend)
    sps = [sp, S(seed=7, stream=1, **PARAMS["k256_p1"])]

    def neighbours():
        one, n_one = s1.resident_decode_sampled(THS.FIRST, THS.PROMPT_LEN, THS.N, sp)
        logits = _download(hip_backend, s1.handle, m1.buf("logits"), V)
        picks = [hip_backend.sample(s1.handle, m1.buf("logits"), 0, V, sp, pos) for pos in range(8)]
        assert [t for t, _ in picks] == [c_sample(logits, sp, pos) for pos in range(8)]
        many, n_many = sb.resident_decode_batch_sampled([1, 2], [0, 0], 12, sps)
        assert not hip_backend.last_error(), hip_backend.last_error()
        return one.tolist(), n_one, picks, many.tolist(), np.asarray(n_many).tolist()

    before = neighbours()
    assert before[0] == want and before[1] == THS.N
    st, mt = spec_session(hip_backend, cfg, T)
    toks, produced, _ = st.resident_decode_speculative_sampled(FIRST_AT_0, 0, N, sp)
    assert produced == N and np.all(toks >= 0) and not hip_backend.last_error()
    assert neighbours() == before
    for x in (st, mt, s1, m1, sb, bm):
        x.close()


# ── 8. Llama-2-7B dimensions ───────────────────────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("small_m", [1, 0])
def test_l7_dimensions_device_loop_equals_the_host_driven_loop(hip_backend, small_m):
    """Two layers at Llama-2-7B dimensions, T = 4, 12 tokens: vocab 32000 is 18 slices per row, and the synthetic head's ~112 distinct
    logit values per row make the candidate order's index rule decide most ranks. With ZGML_HIP_OPT_SMALL_M_MATVEC = 1 the verify
    step's projections take the multi-row K-on-lanes kernel, without it the tile kernels."""
    T, n, first = 4, 12, 20000
    cfg, sp = l7cfg(2), S(1.0, 40, 0.9, seed=31, stream=4)
    s, m = spec_session(hip_backend, cfg, T, small_m=small_m, threads=16)
    assert ("qmatvec-kon-rows" in hip_backend.planText(s.handle)) == bool(small_m)
    host = Host(hip_backend, cfg, T, 0, small_m=small_m, threads=16)
    assert ("qmatvec-kon-rows" in hip_backend.planText(host.s.handle)) == bool(small_m)
    rows = host.rows_fn(sp)
    want, produced, want_stats = SSM.spec_loop(rows, first, 0, n, T)
    assert produced == n
    right = want + want[-1:] * T
    wrong = [(t + 1) % cfg.vocab_size if i in (2, 7) else t for i, t in enumerate(right)]
    assert [i for i in range(len(right)) if right[i] != wrong[i]] == [2, 7]
    for drafts in (None, right, wrong):
        if drafts is not None:
            want2, _, want_stats = SSM.spec_loop(rows, first, 0, n, T, drafts=drafts)
            assert want2 == want
        toks, got_n, stats = s.resident_decode_speculative_sampled(first, 0, n, sp, drafts=drafts)
        assert not hip_backend.last_error(), hip_backend.last_error()
        print(small_m, stats)
        assert toks.tolist() == want and got_n == n and stats == want_stats
    for x in (s, m, host):
        x.close()
