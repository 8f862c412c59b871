"""Seeded top-k / top-p sampling on the MI355X (include/zgml_hip.h: zgml_hip_sample, zgml_hip_resident_decode_sampled,
zgml_hip_resident_decode_batch_sampled; kernels: zgml_amd/csrc/sample.hip).

Every comparison is bit-exact token equality: the device's pick against zgml_amd/csrc/sample.h — the same functions, compiled
for the host into tests/cpp/sample_probe.cpp — applied to the same logits bits. No tolerance, no tie condition. A resident loop is
compared with the same plan driven from the host: Session.step -> downloaded logits -> probe -> next token."""
import ctypes as C

import numpy as np
import pytest

from zgml_amd import DeviceOp, DeviceProgram, ProgramIO, capi, llama
from tests.test_hip_l7dims import l7cfg
from tests.test_sample_host import c_candidates, c_sample

pytestmark = pytest.mark.gpu
f32 = np.float32
S = capi.SamplingC.of

PROMPT_LEN, N = 8, 24
FIRST = 90
PARAMS = {"k40_p95": dict(temperature=0.8, top_k=40, top_p=0.95), "k256_p1": dict(temperature=1.5, top_k=256, top_p=1.0),
          "k1": dict(temperature=0.7, top_k=1, top_p=1.0)}


# ── zgml_hip_sample on crafted vectors ─────────────────────────────────────────────────────────────────────────────────

def plateau_members(n):
    """up to 300 indices: 0, n - 1, then both sides of the multiples of 1024, of 256, of 64"""
    want = [0, n - 1]
    for step in (1024, 256, 64):
        for m in range(step, n, step):
            want += [m - 1, m]
    seen, out = set(), []
    for i in want:
        if 0 <= i < n and i not in seen:
            seen.add(i), out.append(i)
    return sorted(out[:300])


def crafted(n):
    """(name, vector, top_ks, what the candidates must be — a function of k — or None)"""
    rng = np.random.default_rng(n)
    ks = [1, 2, 40, 256]
    plat = rng.standard_normal(n).astype(f32)
    members = plateau_members(n)
    plat[members] = 7.5
    sparse = np.full(n, -np.inf, f32)
    three = sorted({0, n // 2, n - 1})
    sparse[three] = [1.0, 0.25, 1.0][:len(three)]
    zeros = np.where(rng.random(n) < 0.5, 0.0, -0.0).astype(f32)
    return [
        ("normal", rng.standard_normal(n).astype(f32), ks, None),
        ("all_equal", np.full(n, -1.25, f32), ks, lambda k: list(range(min(k, n)))),
        ("plateau", plat, ks, lambda k: members[:k] if k <= len(members) else None),
        ("ramp", np.arange(n, dtype=f32) * f32(0.01), ks, lambda k: list(range(n - 1, max(n - 1 - k, -1), -1))),  # the winners are in the last slice
        ("three_finite", sparse, [40], None),
        ("signed_zeros", zeros, [1], lambda k: [0]),
    ]


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1000, 4097, 49152, 50001])
def test_sample_on_crafted_vectors(hip_backend, n):
    for name, v, ks, expect in crafted(n):
        prog = DeviceProgram(ops=[DeviceOp.elementwise("abs", 1, 0, 0, 1)], buffer_sizes=[v.size, 1], initial_uploads=[ProgramIO(0, v)])
        h = hip_backend.compileProgram(prog)
        for k in ks:
            sp = S(seed=0xC0FFEE + n, stream=k, **({"temperature": 0.8, "top_p": 0.95} if k != 256 else {"temperature": 1.5, "top_p": 1.0}), top_k=k)
            want_cand = c_candidates(v, k)
            if expect is not None and expect(k) is not None:
                assert want_cand == expect(k), (name, n, k)  # (the probe itself, against the pattern's meaning)
            finite = set(np.flatnonzero(np.isfinite(v)).tolist())
            for pos in range(64):
                tok, cand = hip_backend.sample(h, 0, 0, n, sp, pos)
                assert cand == want_cand, f"selection: {name} n={n} k={k} pos={pos}"
                assert tok == c_sample(v, sp, pos), f"pick: {name} n={n} k={k} pos={pos}"
                if name == "three_finite":
                    assert tok in finite
                if name == "signed_zeros":
                    assert tok == hip_backend.argmax(h, 0, 0, n)
            assert not hip_backend.last_error(), hip_backend.last_error()
        hip_backend.freeProgram(h)


def test_sample_of_a_slice_of_the_buffer(hip_backend):
    """offset > 0: the indices are relative to the slice (as zgml_hip_argmax's)"""
    v = np.random.default_rng(4).standard_normal(5000).astype(f32)
    prog = DeviceProgram(ops=[DeviceOp.elementwise("abs", 1, 0, 0, 1)], buffer_sizes=[v.size, 1], initial_uploads=[ProgramIO(0, v)])
    h = hip_backend.compileProgram(prog)
    sp = S(0.9, 40, 0.9, seed=3)
    for pos in range(16):
        tok, cand = hip_backend.sample(h, 0, 1001, 3000, sp, pos)
        assert cand == c_candidates(v[1001:4001], 40) and tok == c_sample(v[1001:4001], sp, pos)
    hip_backend.freeProgram(h)


# ── the resident loop against the host-driven loop on the same plan ────────────────────────────────────────────────────

def tiny():
    return llama.preset("tiny", 64)


def prompt(cfg, n=PROMPT_LEN):
    return [(7 * i + 3) % cfg.vocab_size for i in range(n)]


def session_behind_prompt(be, cfg, start, threads=8):
    m = llama.Model(cfg, llama.Q4_0, threads=threads)
    s = llama.Session(m, llama.hip_backend_fns(be))
    for pos, t in enumerate(prompt(cfg, start)):
        s.step(t, pos, want_logits=False)
    return s, m


_host = {}


def host_loop(be, sp, first=FIRST, start=PROMPT_LEN, n=N):
    """the reference: the decode plan stepped through the vtable, every token sampled on the host from the downloaded logits by the
    header's own functions. Stop tokens are not applied (u depends on the position alone, so a stopped run is a prefix). Computed
    once per parameter set and left unchanged."""
    key = (sp.temperature, sp.top_p, sp.top_k, sp.seed, sp.stream, first, start, n)
    if key not in _host:
        s, m = session_behind_prompt(be, tiny(), start)
        tok, out = first, []
        for pos in range(start, start + n):
            _, logits = s.step(tok, pos)
            tok = c_sample(logits, sp, pos)
            out.append(tok)
        s.close(), m.close()
        _host[key] = out
    return list(_host[key])


def resident(be, start=PROMPT_LEN):
    s, m = session_behind_prompt(be, tiny(), start)
    s.resident_setup(be)
    return s, m


@pytest.mark.parametrize("name", list(PARAMS))
def test_resident_loop_equals_the_host_loop(hip_backend, name):
    sp = S(seed=1234, stream=0, **PARAMS[name])
    want = host_loop(hip_backend, sp)
    s, m = resident(hip_backend)
    got, produced = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, sp)
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert got.tolist() == want and produced == N
    if name == "k1":  # one candidate: the greedy loop
        g, mg = resident(hip_backend)
        assert g.resident_decode(FIRST, PROMPT_LEN, N).tolist() == want
        g.close(), mg.close()
    else:
        assert len(set(want)) > 3  # (it does sample)
    s.close(), m.close()


def test_two_calls_equal_one(hip_backend):
    sp = S(seed=1234, **PARAMS["k40_p95"])
    want = host_loop(hip_backend, sp)
    s, m = resident(hip_backend)
    a, na = s.resident_decode_sampled(FIRST, PROMPT_LEN, 10, sp)
    b, nb = s.resident_decode_sampled(int(a[9]), PROMPT_LEN + 10, 14, sp)
    assert (na, nb) == (10, 14) and a.tolist() + b.tolist() == want
    one, _ = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, sp)
    assert one.tolist() == want
    s.close(), m.close()


def test_seed_and_stream(hip_backend):
    sps = [S(seed=1, stream=0, **PARAMS["k256_p1"]), S(seed=2, stream=0, **PARAMS["k256_p1"]), S(seed=1, stream=1, **PARAMS["k256_p1"]),
           S(seed=1 << 32, stream=0, **PARAMS["k256_p1"])]  # (the last: the seed's high word is a key word of its own)
    wants = [host_loop(hip_backend, sp) for sp in sps]
    for i in range(len(wants)):
        for j in range(i):
            assert wants[i] != wants[j], (i, j)  # precondition: seeds and streams matter to the reference
    s, m = resident(hip_backend)
    for sp, want in zip(sps, wants):
        got, _ = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, sp)  # (one captured graph, four parameter sets)
        assert got.tolist() == want
    s.close(), m.close()


def test_greedy_and_sampled_alternate_on_one_program(hip_backend):
    sp = S(seed=77, **PARAMS["k40_p95"])
    want = host_loop(hip_backend, sp)
    s, m = resident(hip_backend)
    g1 = s.resident_decode(FIRST, PROMPT_LEN, N).tolist()
    got, _ = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, sp)
    g2 = s.resident_decode(FIRST, PROMPT_LEN, N).tolist()
    got2, _ = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, sp)
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert g1 == g2 and got.tolist() == want == got2.tolist()
    assert g1 == host_loop(hip_backend, S(seed=0, **PARAMS["k1"]))
    s.close(), m.close()


def test_stop_token(hip_backend):
    # a reference stream whose token of step 5 has not occurred before (chosen by the reference alone)
    for seed in range(16):
        sp = S(seed=seed, **PARAMS["k256_p1"])
        want = host_loop(hip_backend, sp)
        if want[5] not in want[:5]:
            break
    else:
        pytest.fail("no reference stream emits a new token at step 5")
    stop = want[5]
    sp_stop = S(seed=seed, stop=[stop], **PARAMS["k256_p1"])
    s, m = resident(hip_backend)
    got, produced = s.resident_decode_sampled(FIRST, PROMPT_LEN, N, sp_stop)
    assert produced == 6 and got[:6].tolist() == want[:6] and np.all(got[6:] == -1)
    # from the stop position the generation continues as the reference does
    nxt, n2 = s.resident_decode_sampled(stop, PROMPT_LEN + 6, 10, sp)
    assert n2 == 10 and nxt.tolist() == want[6:16]
    # a stop token at the last step: nothing is left to freeze
    got, produced = s.resident_decode_sampled(FIRST, PROMPT_LEN, 6, sp_stop)
    assert produced == 6 and got.tolist() == want[:6]
    assert not hip_backend.last_error(), hip_backend.last_error()
    s.close(), m.close()


# ── batched ────────────────────────────────────────────────────────────────────────────────────────────────────────────

def test_batched_loop_equals_the_host_driven_loop_on_the_same_plan(hip_backend):
    """B = 3 with their own parameters, streams, start positions and step counts; the reference is the same batched plan stepped
    through the vtable (BatchSession.step), each row sampled on the host. One sequence has a stop token that fires: its row ends
    there, the others are what they are without it."""
    cfg, B = tiny(), 3
    starts, steps, firsts = [0, 3, 5], [12, 9, 7], [90, 292, 22]
    sps = [S(seed=5, stream=0, **PARAMS["k40_p95"]), S(seed=5, stream=1, **PARAMS["k256_p1"]), S(seed=9, stream=2, temperature=1.0, top_k=5, top_p=0.9)]
    p = prompt(cfg)

    def fill(bs):  # the caches behind every start position: sequence b walks its prompt and then repeats the last prompt position
        for j in range(max(starts)):
            pos = [min(j, max(st - 1, 0)) for st in starts]
            bs.step([p[x] for x in pos], pos)

    bm = llama.BatchModel(cfg, B)
    host = llama.BatchSession(bm, llama.hip_backend_fns(hip_backend), B)
    fill(host)
    tok, pos, want = list(firsts), list(starts), [[] for _ in range(B)]
    for i in range(max(steps)):
        _, logits = host.step(tok, pos)  # (a sequence behind its count repeats its step, as the device loop's does)
        for b in range(B):
            if i < steps[b]:
                tok[b] = c_sample(logits[b], sps[b], pos[b])
                pos[b] += 1
                want[b].append(tok[b])
    host.close()
    # sequence 1 stops at the first step >= 2 whose token is new to it
    at = next(i for i in range(2, steps[1]) if want[1][i] not in want[1][:i])
    sps_stop = list(sps)
    sps_stop[1] = S(seed=5, stream=1, stop=[want[1][at]], **PARAMS["k256_p1"])
    dev = llama.BatchSession(bm, llama.hip_backend_fns(hip_backend), B)
    fill(dev)
    dev.resident_setup(hip_backend)
    got, produced = dev.resident_decode_batch_sampled(firsts, starts, steps, sps_stop)
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert produced.tolist() == [steps[0], at + 1, steps[2]]
    for b in range(B):
        n = int(produced[b])
        assert got[b, :n].tolist() == want[b][:n], b
        assert np.all(got[b, n:] == -1)
    # the greedy batched loop and the sampled one alternate on the program; k = 1 rows are the greedy rows
    g1 = dev.resident_decode_batch(firsts, starts, steps)
    k1, _ = dev.resident_decode_batch_sampled(firsts, starts, steps, [S(seed=b, **PARAMS["k1"]) for b in range(B)])
    assert np.array_equal(g1, k1)
    dev.close(), bm.close()


# ── Llama-2-7B dimensions ──────────────────────────────────────────────────────────────────────────────────────────────

def test_l7_dimensions_equal_the_host_loop(hip_backend):
    """vocab 32000 (18 slices), a synthetic head with ~112 distinct logit values per row: ties everywhere, so the candidate
    order's index rule decides most ranks. 8 sampled steps against the same plan stepped from the host."""
    cfg, first, n = l7cfg(2), 20000, 8
    sp = S(1.0, 40, 0.9, seed=31, stream=4)
    m = llama.Model(cfg, llama.Q4_0, threads=16)
    host = llama.Session(m, llama.hip_backend_fns(hip_backend))
    tok, want = first, []
    for pos in range(n):
        _, logits = host.step(tok, pos)
        tok = c_sample(logits, sp, pos)
        want.append(tok)
    s = llama.Session(m, llama.hip_backend_fns(hip_backend))
    s.resident_setup(hip_backend)
    got, produced = s.resident_decode_sampled(first, 0, n, sp)
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert got.tolist() == want and produced == n
    s.close(), host.close(), m.close()


# ── refusals ───────────────────────────────────────────────────────────────────────────────────────────────────────────

def _dispatches(be, handle):
    p = be.getRuntimeProfile(handle)
    return (int(p.backend_dispatch_count), int(p.call_count))


BAD_PARAMS = [(dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"), (dict(temperature=float("nan")), "temperature"),
              (dict(top_p=0.0), "top_p"), (dict(top_p=1.5), "top_p"), (dict(top_p=float("nan")), "top_p"), (dict(top_k=257), "top_k"),
              (dict(stop=[1, 2, 3, 4, 5]), "n_stop")]


def test_refusals_enqueue_nothing_and_the_next_call_works(hip_backend):
    cfg = tiny()
    hip, V, L = capi.load_hip(), cfg.vocab_size, cfg.max_seq_len
    s, m = resident(hip_backend, 0)
    good = S(seed=1, **PARAMS["k40_p95"])
    before = _dispatches(hip_backend, s.handle)

    def refused(call, text):
        with pytest.raises(RuntimeError, match=text):
            call()
        hip.zgml_hip_clear_error(hip_backend.ctx)
        assert _dispatches(hip_backend, s.handle) == before

    for kw, text in BAD_PARAMS + [(dict(stop=[V]), "stop token")]:
        refused(lambda: s.resident_decode_sampled(1, 0, 4, S(**kw)), text)
    refused(lambda: s.resident_decode_sampled(V, 0, 4, good), "out of range")
    refused(lambda: s.resident_decode_sampled(1, L - 3, 4, good), "out of range")
    for kw, text in BAD_PARAMS:  # (zgml_hip_sample does not look at the stop tokens' values)
        refused(lambda: hip_backend.sample(s.handle, m.buf("logits"), 0, V, S(**kw), 0), text)
    refused(lambda: hip_backend.sample(s.handle, m.buf("logits"), 1, V, good, 0), "inside the buffer")
    refused(lambda: hip_backend.sample(s.handle, m.buf("logits"), 0, 0, good, 0), "inside the buffer")
    # a token_len > 1 plan and a batched plan to the single-sequence call; a plain plan to the batched call
    m4 = llama.Model(cfg, llama.Q4_0, token_len=4)
    s4 = llama.Session(m4, llama.hip_backend_fns(hip_backend))
    s4.resident_setup(hip_backend)
    refused(lambda: s4.resident_decode_sampled(1, 0, 4, good), "token_len")
    bm = llama.BatchModel(cfg, 2)
    sb = llama.BatchSession(bm, llama.hip_backend_fns(hip_backend), 2)
    sb.resident_setup(hip_backend)
    out, n_out = np.zeros(4, np.int64), C.c_uint32(0)
    assert hip.zgml_hip_resident_decode_sampled(hip_backend.ctx, sb.handle, 1, 0, 4, C.byref(good), out.ctypes.data, C.byref(n_out)) == -1
    assert "batched" in hip_backend.last_error()
    hip.zgml_hip_clear_error(hip_backend.ctx)
    u32p = C.POINTER(C.c_uint32)
    two = np.array([1, 1], np.uint32)
    sp2 = (capi.SamplingC * 2)(good, good)
    assert hip.zgml_hip_resident_decode_batch_sampled(hip_backend.ctx, s.handle, two.ctypes.data_as(u32p), two.ctypes.data_as(u32p), two.ctypes.data_as(u32p), 1,
                                                      sp2, out.ctypes.data, None) == -1
    assert "not a batched program" in hip_backend.last_error()
    hip.zgml_hip_clear_error(hip_backend.ctx)
    # the batched call: a bad parameter set of one sequence, a position out of range under the greedy loop's rules
    before_b = _dispatches(hip_backend, sb.handle)
    for bad in ([good, S(temperature=0.0)], [S(stop=[V]), good]):
        with pytest.raises(RuntimeError, match="sequence"):
            sb.resident_decode_batch_sampled([1, 1], [0, 0], [2, 2], bad)
        hip.zgml_hip_clear_error(hip_backend.ctx)
    with pytest.raises(RuntimeError, match="out of range"):
        sb.resident_decode_batch_sampled([1, 1], [0, L - 2], [3, 2], [good, good])  # (sequence 1 would idle at max_seq)
    hip.zgml_hip_clear_error(hip_backend.ctx)
    assert _dispatches(hip_backend, sb.handle) == before_b
    # the next valid calls work
    got, produced = s.resident_decode_sampled(FIRST, 0, N, good)
    assert produced == N and got.tolist() == host_loop(hip_backend, good, FIRST, 0, N)
    toks, produced = sb.resident_decode_batch_sampled([1, 1], [0, 0], [3, 3], [good, good])
    assert produced.tolist() == [3, 3] and np.all(toks >= 0) and not hip_backend.last_error()
    for x in (s, m, s4, m4, sb, bm):
        x.close()
