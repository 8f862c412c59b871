"""Batched decode over per-sequence int8 KV caches on the MI355X (BatchModel(..., kv_quant_block=32)): against the oracle over the
oracle's greedy tokens (bound and token rule: tests/kvq_cases.py), the launch plan's shape at Llama-2-7B dimensions (one
decode-attention launch per layer carrying every head of every sequence in the int8 form), and the device-resident loops — greedy,
and sampled with log-probabilities and a token automaton — against stepping the same plan."""
import numpy as np
import pytest

from zgml_amd import ProgramIO, capi, llama
from zgml_amd.program import ios_to_c
from tests.kvq_cases import check_against_trace, oracle_trace
from tests.test_constraint_host import Dfa, FORBIDDEN
from tests.test_hip_batch_decode import launches, plan_text, stepped_tokens
from tests.test_hip_l7dims import l7cfg

pytestmark = pytest.mark.gpu
f32 = np.float32
S = capi.SamplingC.of


@pytest.mark.parametrize("kind", [llama.Q4_0, llama.Q8_0])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("B", [2, 3])
def test_tiny_int8_batch_matches_oracle(hip_backend, oracle, B, fused, kind):
    bm = llama.BatchModel(llama.preset("tiny"), B, kind, fused_elementwise=fused, include_dead_f32=True, kv_quant_block=32)
    s_ref = llama.BatchSession(bm, oracle.backend_fns(), B)
    trace = oracle_trace(s_ref, [9, 43, 465][:B], [0, 5, 2][:B], 8)  # (first tokens whose 8 greedy rows are all decisive on the oracle, either kind)
    s_hip = llama.BatchSession(bm, llama.hip_backend_fns(hip_backend), B)
    print("worst, decisive, rows:", check_against_trace(hip_backend, s_hip, trace))
    s_hip.close(), s_ref.close(), bm.close()


def download(be, handle, buf, n_elems):
    out = np.zeros(n_elems, f32)
    capi.load_hip().zgml_hip_download_outputs(be.ctx, handle, ios_to_c([ProgramIO(buf, out)]), 1)
    assert not be.last_error(), be.last_error()
    return out


@pytest.mark.parametrize("B", [2, 4])
def test_l7_dimensions_sequence_0_admitted_past_the_split_threshold(hip_backend, oracle, B):
    """Llama-2-7B dimensions, two layers, the LM head tied to the embedding: the synthetic quantized head repeats columns (32000
    logits, 112 distinct values, every maximum an exact tie), the sin / cos embedding does not, so the oracle has decisive rows.
    Sequence 0 starts at position 300 — past the attention-split threshold, so its heads' context is split over several workgroups
    while the other sequences' (position 0) is not, in the same launch — over a 300-token prompt prefilled on the f32 T-token plan
    of the same weights (three chunks of 100, on the device) and admitted into its int8 caches through zgml_hip_kv_move. The
    oracle's slot gets the same f32 columns, downloaded from the prefill plan, through its own quantizeInput (the prefill has its
    own tests; the oracle takes 20 s over one). ZGML_HIP_OPT_SMALL_M_MATVEC on (the multi-row mat-vec) and off (the tile kernels).
    First tokens, from the series (911 b + 17) mod vocab of tests/test_hip_batch_decode.py, chosen on the oracle alone: sequence 0
    takes the first member whose four greedy rows at positions 300..303 behind the prompt are decisive, the others the first
    members whose four rows from position 0 are."""
    be, n_pre, chunk = hip_backend, 300, 100
    oracle.set_threads(16)
    cfg = l7cfg(2)
    cfg.tied_lm_head = 1
    dh, S_ = cfg.d_head, cfg.max_seq_len
    base = llama.Model(cfg, llama.Q4_0, threads=16)
    bm = llama.BatchModel(None, B, like=base, kv_quant_block=32)
    mp = llama.Model(None, token_len=chunk, like=base)  # the f32 T-token plan whose caches are handed over
    fns = llama.hip_backend_fns(be)
    pre = llama.Session(mp, fns)
    prompt = [(31 * j + 7) % cfg.vocab_size for j in range(n_pre)]
    for p in range(0, n_pre, chunk):
        pre.prefill(prompt[p:p + chunk], p, want_logits=False)
    assert not be.last_error(), be.last_error()
    images = {buf: download(be, pre.handle, buf, n) for buf, n in mp.kv_buffers()}
    # the oracle's slot 0: every lane's first n_pre columns, quantised block by block as storeColumn does
    s_ref = llama.BatchSession(bm, oracle.backend_fns(), B)
    ob = oracle.OracleBackend()
    for ls, ld in zip(mp.kv_lanes(), bm.kv_lanes(0)):
        q, sc = oracle.quantize_input(images[ls.buf][ls.offset:ls.offset + n_pre * dh], 32)
        cache = ob.buffer(s_ref.handle, ld.buf)
        cache.view(np.int8)[:n_pre * dh] = q
        cache[S_ * dh // 4:S_ * dh // 4 + n_pre * dh // 32] = sc
    tokens = [3661, 928, 1839, 4572][:B]
    trace = oracle_trace(s_ref, tokens, [n_pre] + [0] * (B - 1), 4)
    s_ref.close()
    for small_m in (8, False):
        s_hip = llama.BatchSession(bm, fns, B, small_m_matvec=small_m)
        s_hip.admit(0, pre, n_pre)
        print("small_m", small_m, "worst, decisive, rows:", check_against_trace(be, s_hip, trace))
        s_hip.close()
    pre.close(), mp.close(), bm.close(), base.close()


def test_plan_shape_at_7b_dimensions_int8(hip_backend):
    """Per layer ONE decode-attention launch carrying the B * 32 head records in the int8 form (ropes, kvq stores, attention_kvq and
    row store of every head of every sequence folded: 6 ops per head at n_kv = n_heads), and no kvq_store / attention_kvq launch of
    its own anywhere: the plan of the f32 batched program (tests/test_hip_batch_decode.py), 11 launches per layer."""
    B, L = 4, 2
    cfg = l7cfg(L)
    bm = llama.BatchModel(cfg, B, llama.Q4_0, threads=16, kv_quant_block=32)
    s = llama.BatchSession(bm, llama.hip_backend_fns(hip_backend), B)
    text = plan_text(hip_backend, s.handle)
    ls = launches(text)
    K = capi.DOP
    assert not [l for l in ls if l[0] in (K["kvq_store"], K["attention_kvq"])], text
    adec = [l for l in ls if "decode-attention" in l[4]]
    assert len(adec) == L, text
    H, KV = cfg.n_heads, cfg.n_kv_heads
    assert all(l[1] == B * (3 * KV + 3 * H) and f"heads {B * H} kvq" in l[4] for l in adec), text
    layer = [K["rmsnorm"], K["qmatmul"], K["qmatmul"], K["qmatmul"], K["attention"], K["qmatmul"], K["rmsnorm"], K["qmatmul"], K["qmatmul"],
             K["fused_elementwise"], K["qmatmul"]]
    assert [l[0] for l in ls] == layer * L + [K["rmsnorm"], K["qmatmul"]], text
    s.close(), bm.close()


@pytest.mark.parametrize("name,kind", [("tiny", llama.Q4_0), ("tiny", llama.Q8_0), ("smollm-135m", llama.Q4_0)])
def test_resident_batch_equals_stepping_int8(hip_backend, name, kind):
    """zgml_hip_resident_decode_batch over the int8 plan against stepping the same plan through refresh_dynamic_batch: identical
    tokens for full, ragged and resumed calls."""
    B, n = 3, (16 if name == "tiny" else 8)
    bm = llama.BatchModel(llama.preset(name), B, kind, threads=8, kv_quant_block=32)
    s = llama.BatchSession(bm, llama.hip_backend_fns(hip_backend), B)
    s.use_dynamic_refresh()
    first, start = [5, 90, 33], [0, 3, 1]
    s.resident_setup(hip_backend)
    got = s.resident_decode_batch(first, start, n)  # the program's first execution is the resident loop
    assert not hip_backend.last_error(), hip_backend.last_error()
    want = stepped_tokens(s, first, start, [n] * B)
    assert got.tolist() == want.tolist()
    counts = [n, n // 2, 1]
    ragged = s.resident_decode_batch(first, start, counts)
    assert ragged.shape == (B, n)
    for b in range(B):
        assert ragged[b, :counts[b]].tolist() == want[b, :counts[b]].tolist() and np.all(ragged[b, counts[b]:] == -1)
    full = s.resident_decode_batch(first, start, n)
    assert full.tolist() == want.tolist()
    h = n // 2
    resumed = s.resident_decode_batch(want[:, h - 1], [p + h for p in start], n - h)
    assert resumed.tolist() == want[:, h:].tolist()
    again = stepped_tokens(s, first, start, [n] * B)
    assert again.tolist() == want.tolist()
    assert not hip_backend.last_error(), hip_backend.last_error()
    s.close(), bm.close()


def test_sampled_with_logprobs_and_a_constraint_equals_the_call_split_in_two(hip_backend):
    be, cfg, B, n, h = hip_backend, llama.preset("tiny"), 3, 14, 6
    V = cfg.vocab_size
    # sequence 1 runs under an automaton over 5 hashed classes: about a third of the transitions forbidden, no dead state
    rng = np.random.default_rng(3)
    nxt = rng.integers(0, 4, (4, 5)).astype(np.uint16)
    nxt[rng.random((4, 5)) < 0.35] = FORBIDDEN
    for st in range(4):
        nxt[st, st] = (st + 1) % 4
    i = np.arange(V, dtype=np.uint64)
    dfa = Dfa((((i * np.uint64(2654435761)) >> np.uint64(7)) % np.uint64(5)).astype(np.uint16), nxt)
    bm = llama.BatchModel(cfg, B, llama.Q4_0, kv_quant_block=32)
    s = llama.BatchSession(bm, llama.hip_backend_fns(be), B)
    s.resident_setup(be)
    con = be.constraint_create(dfa.class_of, dfa.next)
    sps = [S(temperature=0.9, top_k=40, top_p=0.95, seed=5, stream=b) for b in range(B)]
    first, start = [90, 292, 22], [0, 2, 1]
    s.set_constraint(con, 1, seq=1)
    plain, _ = s.resident_decode_batch_sampled(first, start, n, [S(temperature=0.9, top_k=40, top_p=0.95, seed=5, stream=b) for b in range(B)])
    s.set_constraint(None, seq=1)
    free, _ = s.resident_decode_batch_sampled(first, start, n, sps)
    assert free[1].tolist() != plain[1].tolist() and free[0].tolist() == plain[0].tolist()  # the automaton decided something
    s.set_constraint(con, 1, seq=1)
    toks, produced, lps = s.resident_decode_batch_sampled(first, start, n, sps, logprobs=True)
    assert produced.tolist() == [n] * B and toks.tolist() == plain.tolist() and np.isfinite(lps).all() and np.all(lps <= 0)
    state_full = s.constraint_state(1)
    s.set_constraint(con, 1, seq=1)
    a, pa, la = s.resident_decode_batch_sampled(first, start, h, sps, logprobs=True)
    b_, pb, lb = s.resident_decode_batch_sampled(a[:, h - 1], [p + h for p in start], n - h, sps, logprobs=True)  # (the state persists)
    assert pa.tolist() == [h] * B and pb.tolist() == [n - h] * B
    assert np.concatenate([a, b_], axis=1).tolist() == toks.tolist()
    assert np.array_equal(np.concatenate([la, lb], axis=1).view(np.uint32), lps.view(np.uint32))
    assert s.constraint_state(1) == state_full
    assert not be.last_error(), be.last_error()
    s.set_constraint(None, seq=1)
    s.close(), bm.close()
    be.constraint_free(con)
